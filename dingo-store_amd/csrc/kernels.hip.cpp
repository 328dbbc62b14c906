// kernels.hip.cpp — CDNA4 (gfx950) kernels for the dingo-store vector-search
// hot path.  Net-new MI355X-native code (the reference is CPU-only; the
// faiss math it delegates to is restated from SURVEY.md §8a semantics).
//
// Design:
//  * The hot path is HBM-bound (SURVEY.md §8d cfg C): every kernel reads the
//    database stream with 16 B/lane coalesced float4 loads, wave(64)-per-row.
//  * ivf_scan reads each probed list's chunk exactly ONCE per query batch
//    (query tiles staged in LDS, looped inside the kernel), which makes the
//    algorithmic-bytes accounting the achievable ideal.
//  * Candidates and top-k entries are packed (monotone-mapped f32 key << 32
//    | row) into one u64 so selection is a single integer compare and ties
//    break deterministically toward the smaller row.
//  * Plain library GEMMs (query x centroid / query x database dots) go
//    through rocBLAS from the host side (dg_abi.cpp); everything irregular
//    is hand-written here.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dg_internal.h"
#include "dg_shard_core.h"
#include "dg_sq8_core.h"

#define WAVE 64

// ---------- float <-> order-preserving u32 ----------
__device__ __forceinline__ uint32_t enc_f32(float x) {
  uint32_t u = __float_as_uint(x);
  return (int32_t)u < 0 ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_f32(uint32_t e) {
  uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
  return __uint_as_float(u);
}
__device__ __forceinline__ uint64_t pack_cand(float key, uint32_t row) {
  return ((uint64_t)enc_f32(key) << 32) | row;
}
static constexpr uint64_t kCandEmpty = ~0ull;

// ---------- small utilities ----------
__global__ void k_iota_i32(int32_t* p, int64_t n, int32_t v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void k_row_norms(const float* __restrict__ x, int64_t n, int32_t d,
                            float* __restrict__ out) {
  // one wave per row, float4 coalesced
  int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  if (row >= n) return;
  const float* v = x + row * d;
  float acc = 0.f;
  int d4 = d / 4;
  const float4* v4 = (const float4*)v;
  for (int i = lane; i < d4; i += WAVE) {
    float4 a = v4[i];
    acc += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
  }
  for (int i = d4 * 4 + lane; i < d; i += WAVE) acc += v[i] * v[i];
  for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  if (lane == 0) out[row] = acc;
}

__global__ void k_normalize_rows(float* __restrict__ x, int64_t n, int32_t d) {
  // NormalizeVectorForFaiss semantics (vector_index_utils.cc:480-491):
  // double-accumulated norm (distances_ref.cc:62-66), skip when
  // |1 - norm^2| <= 1e-5 or norm^2 == 0.
  int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  if (row >= n) return;
  float* v = x + row * d;
  double acc = 0.0;
  for (int i = lane; i < d; i += WAVE) acc += (double)v[i] * v[i];
  for (int off = 32; off; off >>= 1) acc += __shfl_xor(acc, off, WAVE);
  float n2 = (float)acc;
  if (n2 > 0.f && fabsf(1.0f - n2) > 0.00001f) {
    float inv = 1.0f / sqrtf(n2);
    for (int i = lane; i < d; i += WAVE) v[i] = v[i] * inv;
  }
}

__global__ void k_argmin_rows(const float* __restrict__ dots,
                              const float* __restrict__ cnorms, int64_t n,
                              int32_t nlist, int metric,
                              int32_t* __restrict__ out) {
  // key: L2 = cnorm - 2*dot (qnorm constant per row); IP/COS = -dot.
  // tie: smaller list id (matches oracle strict '<').
  int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  if (row >= n) return;
  const float* dr = dots + row * nlist;
  uint64_t best = kCandEmpty;
  for (int l = lane; l < nlist; l += WAVE) {
    float key = (metric == 0) ? cnorms[l] - 2.0f * dr[l] : -dr[l];
    uint64_t c = pack_cand(key, (uint32_t)l);
    best = min(best, c);
  }
  for (int off = 32; off; off >>= 1)
    best = min(best, (uint64_t)__shfl_xor((long long)best, off, WAVE));
  if (lane == 0) out[row] = (int32_t)(best & 0xffffffffu);
}

// ---------- filter ----------
__device__ bool filter_pass(const dg_dev_filter f, int64_t id) {
  bool in;
  switch (f.kind) {
    case DG_FILTER_RANGE:
      in = (id >= f.min_id && id < f.max_id);  // vector_index.h:77-80
      break;
    case DG_FILTER_SORTED_IDS: {
      int64_t lo = 0, hi = f.n_ids - 1;
      in = false;
      while (lo <= hi) {  // SortFilterFunctor binary search,
        int64_t mid = (lo + hi) >> 1;  // vector_index.h:117-133
        int64_t v = f.ids[mid];
        if (v == id) { in = true; break; }
        if (id < v) hi = mid - 1; else lo = mid + 1;
      }
      break;
    }
    case DG_FILTER_BITMAP: {
      int64_t b = id - f.bitmap_base;
      in = (b >= 0 && b < f.bitmap_nbits) &&
           ((f.bitmap[b >> 6] >> (b & 63)) & 1);
      break;
    }
    default:
      in = true;
      return in;  // NONE: negate does not apply
  }
  return f.negate ? !in : in;
}

__global__ void k_build_pass_bitmap(const int64_t* __restrict__ ids, int64_t n,
                                    dg_dev_filter f,
                                    uint32_t* __restrict__ bitmap) {
  // bit per csr row: filter(id) && not tombstone (id >= 0)
  int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // word index
  int64_t nwords = (n + 31) / 32;
  if (w >= nwords) return;
  uint32_t bits = 0;
  for (int b = 0; b < 32; b++) {
    int64_t row = w * 32 + b;
    if (row < n) {
      int64_t id = ids[row];
      if (id >= 0 && filter_pass(f, id)) bits |= (1u << b);
    }
  }
  bitmap[w] = bits;
}

// ---------- generic block top-k over u64 candidates ----------
// Per-thread sorted ascending list in LDS, guarded insert, then ping-pong
// tree merge.  Dynamic LDS: 2 * T * k * 8 bytes.
__device__ void topk_insert(uint64_t* arr, int32_t& cnt, int32_t k,
                            uint64_t c) {
  if (cnt == k && c >= arr[k - 1]) return;
  int32_t pos = (cnt < k) ? cnt : k - 1;
  while (pos > 0 && arr[pos - 1] > c) {
    arr[pos] = arr[pos - 1];
    pos--;
  }
  arr[pos] = c;
  if (cnt < k) cnt++;
}

__device__ void topk_merge_block(uint64_t* lds, int32_t k, int32_t cnt,
                                 uint64_t* out_row /* k u64, thread 0 */) {
  // lds layout: [2][T][k]; each thread's list sorted asc, padded kCandEmpty
  const int T = blockDim.x;
  const int tid = threadIdx.x;
  uint64_t* a = lds;
  uint64_t* b = lds + (size_t)T * k;
  // pad own list
  for (int i = cnt; i < k; i++) a[(size_t)tid * k + i] = kCandEmpty;
  __syncthreads();
  int src_is_a = 1;
  for (int step = 1; step < T; step *= 2) {
    uint64_t* s = src_is_a ? a : b;
    uint64_t* d = src_is_a ? b : a;
    if ((tid & (2 * step - 1)) == 0 && tid + step < T) {
      const uint64_t* x = s + (size_t)tid * k;
      const uint64_t* y = s + (size_t)(tid + step) * k;
      uint64_t* o = d + (size_t)tid * k;
      int xi = 0, yi = 0;
      for (int i = 0; i < k; i++)
        o[i] = (yi >= k || (xi < k && x[xi] <= y[yi])) ? x[xi++] : y[yi++];
    } else if ((tid & (2 * step - 1)) == 0) {
      // no partner: copy through
      const uint64_t* x = s + (size_t)tid * k;
      uint64_t* o = d + (size_t)tid * k;
      for (int i = 0; i < k; i++) o[i] = x[i];
    }
    src_is_a ^= 1;
    __syncthreads();
  }
  if (tid == 0) {
    uint64_t* s = (src_is_a ? a : b);
    for (int i = 0; i < k; i++) out_row[i] = s[i];
  }
}

// The selection key of a dense score: mode 0 key=score, 1 key=cnorm-2*score,
// 2 key=-score.  One definition for k_select_dense and k_coarse_select, so
// that floating-point contraction gives both the same bits.
__device__ __forceinline__ float select_key_v(int mode, float cn, float s) {
  return (mode == 0) ? s : (mode == 1) ? cn - 2.0f * s : -s;
}
__device__ __forceinline__ float select_key(int mode,
                                            const float* __restrict__ cn,
                                            int64_t c, float s) {
  return select_key_v(mode, mode == 1 ? cn[c] : 0.0f, s);
}

// dense scores row scan: mode 0 key=score, 1 key=cnorm[col]-2*score,
// 2 key=-score.  col_base added to the packed payload (and is the global
// column index for the bitmap); cnorms is indexed by the local column.
// ld = row stride of scores.  blockIdx.y picks a seg_w-wide column segment
// (the wide-k path runs (rows x S) blocks, writing k per segment at
// out_offset + y*k, merged afterwards with select_u64); plain callers
// launch gridDim.y = 1 with seg_w = cols.
__global__ void k_select_dense(const float* __restrict__ scores,
                               const float* __restrict__ cnorms, int64_t rows,
                               int64_t cols, int64_t ld, int64_t seg_w,
                               int32_t k, int mode,
                               const uint32_t* __restrict__ bitmap,
                               int64_t col_base,
                               uint64_t* __restrict__ out,
                               int64_t out_stride, int64_t out_offset) {
  extern __shared__ uint64_t lds[];
  int64_t row = blockIdx.x;
  if (row >= rows) return;
  const int64_t seg_start = (int64_t)blockIdx.y * seg_w;
  const int64_t cseg = min(seg_w, cols - seg_start);
  const float* sr = scores + row * ld + seg_start;
  const float* cn = cnorms + seg_start;
  uint64_t* mine = lds + (size_t)threadIdx.x * k;
  int32_t cnt = 0;
  for (int64_t c = threadIdx.x; c < cseg; c += blockDim.x) {
    if (bitmap) {
      int64_t g = col_base + seg_start + c;
      if (!((bitmap[g >> 5] >> (g & 31)) & 1)) continue;
    }
    float key = select_key(mode, cn, c, sr[c]);
    topk_insert(mine, cnt, k,
                pack_cand(key, (uint32_t)(col_base + seg_start + c)));
  }
  topk_merge_block(lds, k, cnt,
                   out + row * out_stride + out_offset + blockIdx.y * k);
}

// candidate (u64) segment scan per query.  ulen >= 0: every query's segment
// is ulen long and starts at q * ulen (base and total are not read).
__global__ void k_select_u64(const uint64_t* __restrict__ cand,
                             const int64_t* __restrict__ base,
                             const int64_t* __restrict__ total, int64_t ulen,
                             int64_t nq, int32_t k,
                             uint64_t* __restrict__ out,
                             int64_t out_stride) {
  extern __shared__ uint64_t lds[];
  int64_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t* seg =
      cand + (ulen >= 0 ? q * ulen : base ? base[q] : q * total[0]);
  int64_t len = ulen >= 0 ? ulen : base ? total[q] : total[0];
  uint64_t* mine = lds + (size_t)threadIdx.x * k;
  int32_t cnt = 0;
  for (int64_t i = threadIdx.x; i < len; i += blockDim.x)
    topk_insert(mine, cnt, k, seg[i]);
  topk_merge_block(lds, k, cnt, out + q * out_stride);
}

// emit: unpack sorted u64 topk -> faiss-convention distances + resolved ids
__global__ void k_emit(const uint64_t* __restrict__ topk,
                       const int64_t* __restrict__ ids_lookup,
                       const float* __restrict__ qnorms, int64_t nq, int32_t k,
                       int metric, int add_qnorm, float* __restrict__ out_dist,
                       int64_t* __restrict__ out_ids) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * k) return;
  int64_t q = i / k;
  uint64_t c = topk[i];
  if (c == kCandEmpty) {
    out_dist[i] = 0.0f;  // matches oracle topk_emit padding
    out_ids[i] = -1;
    return;
  }
  float key = dec_f32((uint32_t)(c >> 32));
  uint32_t row = (uint32_t)c;
  float dist;
  if (metric == 0) {  // L2: key may be cnorm-2dot; add qnorm back
    dist = add_qnorm ? key + qnorms[q] : key;
    if (dist < 0.f) dist = 0.f;  // clamp fp cancellation, faiss-style
  } else {
    dist = -key;  // raw IP score
  }
  out_dist[i] = dist;
  out_ids[i] = ids_lookup ? ids_lookup[row] : (int64_t)row;
}

// ---------- merge of best-first lists (sharded index, dg_merge_topk) ----------
// dists / ids: [n_lists][nq][k_in], every list sorted under the order of
// dg_shard_core.h.  One thread per input element (q, s, p), p fastest, so a
// wave's own element loads are consecutive in one list.  The thread finds its
// element's final rank with one binary search per other list (dg_merge_rank)
// and, if rank < k_out, writes it to out[q][rank].  The order is total, so
// the ranks of a query are a permutation: no two threads write one slot and
// the kernel needs no atomics, LDS or barriers.  Slots at or beyond
// n_lists * k_in exist only if k_out is larger; the same threads fill them
// with pads, strided by the element count.
__global__ void __launch_bounds__(256)
k_merge_lists(const float* __restrict__ dists, const int64_t* __restrict__ ids,
              int32_t n_lists, int64_t nq, int32_t k_in, int32_t k_out,
              int32_t metric, float* __restrict__ out_dist,
              int64_t* __restrict__ out_ids) {
  const int64_t per_q = (int64_t)n_lists * k_in;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nq * per_q) return;
  const int64_t q = g / per_q;
  const int32_t j = (int32_t)(g - q * per_q);  // element within the query
  const int32_t s = j / k_in, p = j - s * k_in;
  const int64_t rank =
      dg_merge_rank(dists, ids, n_lists, nq, k_in, metric, q, s, p);
  if (rank < k_out) {
    const int64_t self = dg_merge_list_base(nq, k_in, q, s) + p;
    const int64_t id = ids[self];
    const int64_t o = q * k_out + rank;
    out_dist[o] = id < 0 ? 0.0f : dists[self];  // real: bits copied
    out_ids[o] = id < 0 ? -1 : id;
  }
  for (int64_t r = per_q + j; r < k_out; r += per_q) {
    out_dist[q * k_out + r] = 0.0f;
    out_ids[q * k_out + r] = -1;
  }
}

// ---------- IVF probe machinery ----------
__global__ void k_probe_unpack(const uint64_t* __restrict__ topk, int64_t nq,
                               int32_t nprobe, const uint8_t* mask,
                               int32_t* __restrict__ probes) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * nprobe) return;
  uint64_t c = topk[i];
  int32_t l = (c == kCandEmpty) ? -1 : (int32_t)(c & 0xffffffffu);
  if (l >= 0 && mask && !mask[l]) l = -1;  // list-sharding ownership
  probes[i] = l;
}

__global__ void k_probes_all(int64_t nq, int32_t nprobe, const uint8_t* mask,
                             int32_t* __restrict__ probes) {
  // nprobe == nlist: probe every list in id order (no coarse selection)
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * nprobe) return;
  int32_t l = (int32_t)(i % nprobe);
  if (mask && !mask[l]) l = -1;
  probes[i] = l;
}

__global__ void k_hist_probes(const int32_t* __restrict__ probes, int64_t n,
                              int32_t* __restrict__ counts) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t l = probes[i];
  if (l >= 0) atomicAdd(&counts[l], 1);
}

__global__ void k_scatter_probes(const int32_t* __restrict__ probes,
                                 int64_t nq, int32_t nprobe,
                                 int32_t* __restrict__ cursors,
                                 int32_t* __restrict__ inv_q,
                                 int32_t* __restrict__ inv_rank) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * nprobe) return;
  int32_t l = probes[i];
  if (l < 0) return;
  int32_t pos = atomicAdd(&cursors[l], 1);
  inv_q[pos] = (int32_t)(i / nprobe);
  inv_rank[pos] = (int32_t)(i % nprobe);
}

// ---------- coarse probe selection in one kernel ----------
// One block of 4 waves per query picks the np smallest packed keys
// (enc_f32(key) << 32 | list) of a row of nlist coarse scores and writes the
// probe list itself, in ascending key order (DESIGN.md §Coarse probe
// selection).  It is an MSB-first radix select over the 64-bit packed key,
// one byte per pass:
//   - a pass histograms byte b of the keys whose higher bytes equal the
//     prefix chosen so far (256 LDS counters), wave 0 scans the counters and
//     finds the bin that holds the need-th smallest, which extends the
//     prefix; keys below the prefix are in for good;
//   - the packed keys of a row are distinct (the list id is part of them), so
//     a pass whose chosen bin holds exactly `need` keys ends the select: the
//     np keys with (key >> 8b) <= (prefix >> 8b) are the answer.  Byte 0 always
//     ends it.  With distinct scores that is the 3rd or 4th pass; the list-id
//     bytes are only reached through equal scores at the np-th place, and
//     those above nlist's width are skipped (they are zero in every key);
//   - the np survivors go to LDS in arrival order and each of the first np
//     threads ranks its own by counting the smaller ones (np <= 128 broadcast
//     reads), writes probes[q][rank] (masked lists as -1) and counts the
//     probe into the per-list histogram that k_hist_probes would build.
// The row is re-read from L2 in every pass (16 KB at nlist 4096) with float4
// loads when rows are 16-byte aligned (nlist % 4 == 0).  A wave whose lanes
// all hit one counter (the exponent byte, as a rule) adds once.
__global__ void __launch_bounds__(kCoarseWaveThreads)
k_coarse_select(const float* __restrict__ dots,
                const float* __restrict__ cnorms, int32_t nlist, int32_t np,
                int mode, const uint8_t* __restrict__ mask,
                int32_t* __restrict__ probes, int32_t* __restrict__ counts) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t surv[kCoarseWaveMaxNp];
  __shared__ uint32_t s_bin, s_need, s_done, s_cnt;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int64_t q = blockIdx.x;
  const float* row = dots + q * nlist;
  const int32_t n4 = (nlist & 3) == 0 ? nlist >> 2 : 0;

  auto for_each_key = [&](auto&& f) {
    for (int32_t g = tid; g < n4; g += kCoarseWaveThreads) {
      const float4 s = ((const float4*)row)[g];
      float4 c = {0.f, 0.f, 0.f, 0.f};
      if (mode == 1) c = ((const float4*)cnorms)[g];
      const uint32_t col = 4u * (uint32_t)g;
      f(pack_cand(select_key_v(mode, c.x, s.x), col));
      f(pack_cand(select_key_v(mode, c.y, s.y), col + 1));
      f(pack_cand(select_key_v(mode, c.z, s.z), col + 2));
      f(pack_cand(select_key_v(mode, c.w, s.w), col + 3));
    }
    for (int32_t c = 4 * n4 + tid; c < nlist; c += kCoarseWaveThreads)
      f(pack_cand(select_key(mode, cnorms, c, row[c]), (uint32_t)c));
  };

  uint64_t prefix = 0;
  uint32_t need = (uint32_t)np;
  int shift = 56;
  for (int b = 7; b >= 0; b--) {
    // list-id bytes above nlist's width are zero in every key
    if (b > 0 && b < 4 && ((uint32_t)(nlist - 1) >> (8 * b)) == 0) continue;
    shift = 8 * b;
    hist[tid] = 0;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for_each_key([&](uint64_t key) {
      // b == 7 has no higher bytes (and a 64-bit shift is undefined)
      if (b == 7 || (key >> (shift + 8)) == (prefix >> (shift + 8))) {
        const uint32_t bin = (uint32_t)(key >> shift) & 255u;
        const uint32_t first = __builtin_amdgcn_readfirstlane(bin);
        const uint64_t act = __ballot(1);
        if (__ballot(bin == first) == act) {
          if (lane == __ffsll((long long)act) - 1)
            atomicAdd(&hist[first], (uint32_t)__popcll(act));
        } else {
          atomicAdd(&hist[bin], 1u);
        }
      }
    });
    __syncthreads();
    if (tid < WAVE) {
      const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1],
                     h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const uint32_t sum = h0 + h1 + h2 + h3;
      uint32_t incl = sum;
      for (int off = 1; off < WAVE; off <<= 1) {
        const uint32_t t = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += t;
      }
      const uint32_t excl = incl - sum;
      if (excl < need && need <= incl) {  // exactly one lane
        uint32_t r = need - excl, j = 0, hj = h0;
        if (r > hj) { r -= hj; j = 1; hj = h1; }
        if (r > hj) { r -= hj; j = 2; hj = h2; }
        if (r > hj) { r -= hj; j = 3; hj = h3; }
        s_bin = 4 * lane + j;
        s_need = r;
        s_done = (hj == r) ? 1u : 0u;
      }
    }
    __syncthreads();
    prefix |= (uint64_t)s_bin << shift;
    need = s_need;
    if (s_done) break;
    // the next pass's stores to hist and s_* follow its own barrier-separated
    // reads: hist is reset before the first barrier of the pass, after every
    // thread has passed the barrier above; s_* are written after the second
  }

  // exactly np keys have (key >> shift) <= (prefix >> shift)
  const uint64_t limit = prefix >> shift;
  for_each_key([&](uint64_t key) {
    if ((key >> shift) <= limit) {
      const uint32_t slot = atomicAdd(&s_cnt, 1u);
      if (slot < (uint32_t)np) surv[slot] = key;
    }
  });
  __syncthreads();
  if (tid < np) {
    const uint64_t key = surv[tid];
    int32_t rank = 0;
    for (int32_t j = 0; j < np; j++) rank += surv[j] < key ? 1 : 0;
    int32_t l = (int32_t)(key & 0xffffffffu);
    if (mask && !mask[l]) l = -1;  // list-sharding ownership
    probes[q * np + rank] = l;
    if (l >= 0) atomicAdd(&counts[l], 1);
  }
}

// exclusive scan of the per-list probe counts in one block: inv_offsets as
// int64 and int32 (nlist + 1 entries, the last is the total) and the scatter
// cursors (nlist entries), which start at the offsets.  Thread t owns the
// dg_inv_offsets_per_thread(nlist) lists from t * per on.
__global__ void __launch_bounds__(kInvOffsetsThreads)
k_inv_offsets(const int32_t* __restrict__ counts, int32_t nlist,
              int64_t* __restrict__ off64, int32_t* __restrict__ off32,
              int32_t* __restrict__ cursors) {
  __shared__ int64_t wsum[kInvOffsetsThreads / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  const int32_t per = dg_inv_offsets_per_thread(nlist);
  const int32_t lo = min(tid * per, nlist), hi = min(lo + per, nlist);
  int64_t sum = 0;
  for (int32_t i = lo; i < hi; i++) sum += counts[i];
  int64_t incl = sum;
  for (int off = 1; off < WAVE; off <<= 1) {
    const int64_t t = __shfl_up(incl, off, WAVE);
    if (lane >= off) incl += t;
  }
  if (lane == WAVE - 1) wsum[w] = incl;
  __syncthreads();
  int64_t run = incl - sum;
  for (int i = 0; i < w; i++) run += wsum[i];
  for (int32_t i = lo; i < hi; i++) {
    off64[i] = run;
    off32[i] = (int32_t)run;
    cursors[i] = (int32_t)run;
    run += counts[i];
  }
  if (tid == kInvOffsetsThreads - 1) {  // its run is the total
    off64[nlist] = run;
    off32[nlist] = (int32_t)run;
  }
}

__global__ void k_cand_offsets(const int32_t* __restrict__ probes, int64_t nq,
                               int32_t nprobe,
                               const int64_t* __restrict__ csr_offsets,
                               int64_t* __restrict__ qp_off,
                               int64_t* __restrict__ q_total) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  int64_t run = 0;
  for (int32_t p = 0; p < nprobe; p++) {
    qp_off[q * nprobe + p] = run;
    int32_t l = probes[q * nprobe + p];
    if (l >= 0) run += csr_offsets[l + 1] - csr_offsets[l];
  }
  q_total[q] = run;
}

__global__ void k_alg_bytes(const int32_t* __restrict__ inv_counts,
                            const int64_t* __restrict__ csr_offsets,
                            int32_t nlist, int64_t row_bytes,
                            int64_t* __restrict__ out) {
  __shared__ long long lds[256];
  long long acc = 0;
  for (int32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < nlist;
       l += gridDim.x * blockDim.x)
    if (inv_counts[l] > 0)
      acc += (csr_offsets[l + 1] - csr_offsets[l]) * row_bytes;
  lds[threadIdx.x] = acc;
  __syncthreads();
  for (int s = blockDim.x / 2; s; s >>= 1) {
    if (threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    atomicAdd((unsigned long long*)out, (unsigned long long)lds[0]);
}

__global__ void k_unit_counts(const int32_t* __restrict__ inv_counts,
                              int32_t nlist,
                              const int64_t* __restrict__ csr_offsets,
                              int32_t chunk_rows,
                              int32_t* __restrict__ unit_counts) {
  int32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlist) return;
  int64_t len = csr_offsets[l + 1] - csr_offsets[l];
  unit_counts[l] =
      (inv_counts[l] > 0 && len > 0) ? (int32_t)((len + chunk_rows - 1) / chunk_rows) : 0;
}

__global__ void k_fill_units(const int32_t* __restrict__ unit_offsets,
                             const int32_t* __restrict__ unit_counts,
                             int32_t nlist, uint32_t* __restrict__ units) {
  int32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlist) return;
  int32_t base = unit_offsets[l];
  for (int32_t c = 0; c < unit_counts[l]; c++) {
    units[2 * (base + c)] = (uint32_t)l;
    units[2 * (base + c) + 1] = (uint32_t)c;
  }
}

// ---------- range search (radius) ----------
// The float kinds admit a row on the very number k_range_emit writes out:
// range_dist() is that number, and count, compact and emit all call it, so
// "admitted" and "emitted dist < radius" (IP / COSINE: score > radius)
// cannot round apart.  Strict comparison, as faiss RangeSearch; a NaN key
// admits nothing.  The count and compact passes must agree bit for bit (the
// compact pass writes at offsets sized by the count pass): both go through
// range_admit() / dense_key() and nothing else.
__device__ __forceinline__ float range_dist(float key, int metric,
                                            int add_qnorm, float qn) {
  if (metric == 0) {  // L2: key may be cnorm-2dot; add qnorm back, clamp
    float dist = add_qnorm ? key + qn : key;
    return dist < 0.f ? 0.f : dist;
  }
  return -key;  // raw IP score
}
__device__ __forceinline__ bool range_admit(float key, int metric, float qn,
                                            float radius) {
  const float dist = range_dist(key, metric, 1, qn);
  return metric == 0 ? dist < radius : dist > radius;
}
// mode as k_select_dense
__device__ __forceinline__ float dense_key(float s, float cn, int mode) {
  return (mode == 0) ? s : (mode == 1) ? cn - 2.0f * s : -s;
}

// candidates (packed u64) of a query within the radius.  thr != nullptr
// (the binary kinds, integer distances): packed key below thr[q], and
// metric / qnorms / radius are unused.  thr == nullptr (the float kinds):
// range_admit on the decoded key; qnorms is read for metric 0 only.
__device__ __forceinline__ bool cand_admit(uint64_t c, bool packed,
                                           uint64_t t, int metric, float qn,
                                           float radius) {
  if (packed) return c < t;
  return c != kCandEmpty &&
         range_admit(dec_f32((uint32_t)(c >> 32)), metric, qn, radius);
}

__global__ void k_count_below(const uint64_t* __restrict__ cand,
                              const int64_t* __restrict__ base,
                              const int64_t* __restrict__ total,
                              const uint64_t* __restrict__ thr, int metric,
                              const float* __restrict__ qnorms, float radius,
                              int64_t nq, int64_t* __restrict__ counts) {
  __shared__ int64_t lds[256];
  int64_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t* seg = cand + base[q];
  const bool packed = thr != nullptr;
  const uint64_t t = packed ? thr[q] : 0;
  const float qn = (!packed && metric == 0) ? qnorms[q] : 0.f;
  int64_t c = 0;
  for (int64_t i = threadIdx.x; i < total[q]; i += blockDim.x)
    if (cand_admit(seg[i], packed, t, metric, qn, radius)) c++;
  lds[threadIdx.x] = c;
  __syncthreads();
  for (int s = blockDim.x / 2; s; s >>= 1) {
    if (threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[q] = lds[0];
}

__global__ void k_compact_below(const uint64_t* __restrict__ cand,
                                const int64_t* __restrict__ base,
                                const int64_t* __restrict__ total,
                                const uint64_t* __restrict__ thr, int metric,
                                const float* __restrict__ qnorms,
                                float radius,
                                const int64_t* __restrict__ out_off,
                                int64_t nq, int64_t* __restrict__ cursors,
                                uint64_t* __restrict__ out) {
  int64_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t* seg = cand + base[q];
  const bool packed = thr != nullptr;
  const uint64_t t = packed ? thr[q] : 0;
  const float qn = (!packed && metric == 0) ? qnorms[q] : 0.f;
  for (int64_t i = threadIdx.x; i < total[q]; i += blockDim.x) {
    uint64_t c = seg[i];
    if (cand_admit(c, packed, t, metric, qn, radius)) {
      int64_t pos = atomicAdd((unsigned long long*)&cursors[q], 1ull);
      out[out_off[q] + pos] = c;  // host sorts per query afterwards
    }
  }
}

// dense (Flat, float kinds) variants over a dots chunk; mode 1 (L2, key =
// cnorm - 2 dot, qnorms read) or 2 (IP / COSINE, key = -dot)
__global__ void k_count_below_dense(const float* __restrict__ scores,
                                    const float* __restrict__ cnorms,
                                    int64_t rows, int64_t cols, int mode,
                                    const uint32_t* __restrict__ bitmap,
                                    int64_t col_base,
                                    const float* __restrict__ qnorms,
                                    float radius,
                                    int64_t* __restrict__ counts) {
  __shared__ int64_t lds[256];
  int64_t row = blockIdx.x;
  if (row >= rows) return;
  const float* sr = scores + row * cols;
  const int metric = mode == 1 ? 0 : 1;
  const float qn = mode == 1 ? qnorms[row] : 0.f;
  int64_t c = 0;
  for (int64_t j = threadIdx.x; j < cols; j += blockDim.x) {
    int64_t g = col_base + j;
    if (bitmap && !((bitmap[g >> 5] >> (g & 31)) & 1)) continue;
    if (range_admit(dense_key(sr[j], cnorms[j], mode), metric, qn, radius))
      c++;
  }
  lds[threadIdx.x] = c;
  __syncthreads();
  for (int s2 = blockDim.x / 2; s2; s2 >>= 1) {
    if (threadIdx.x < s2) lds[threadIdx.x] += lds[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[row] += lds[0];  // accumulates over chunks
}

__global__ void k_compact_below_dense(const float* __restrict__ scores,
                                      const float* __restrict__ cnorms,
                                      int64_t rows, int64_t cols, int mode,
                                      const uint32_t* __restrict__ bitmap,
                                      int64_t col_base,
                                      const float* __restrict__ qnorms,
                                      float radius,
                                      const int64_t* __restrict__ out_off,
                                      int64_t* __restrict__ cursors,
                                      uint64_t* __restrict__ out) {
  int64_t row = blockIdx.x;
  if (row >= rows) return;
  const float* sr = scores + row * cols;
  const int metric = mode == 1 ? 0 : 1;
  const float qn = mode == 1 ? qnorms[row] : 0.f;
  for (int64_t j = threadIdx.x; j < cols; j += blockDim.x) {
    int64_t g = col_base + j;
    if (bitmap && !((bitmap[g >> 5] >> (g & 31)) & 1)) continue;
    const float key = dense_key(sr[j], cnorms[j], mode);
    if (range_admit(key, metric, qn, radius)) {
      int64_t pos = atomicAdd((unsigned long long*)&cursors[row], 1ull);
      out[out_off[row] + pos] = pack_cand(key, (uint32_t)g);
    }
  }
}

__global__ void k_range_emit(const uint64_t* __restrict__ packed,
                             const int64_t* __restrict__ lims,
                             const int64_t* __restrict__ ids_lookup,
                             const float* __restrict__ qnorms, int64_t nq,
                             int metric, int add_qnorm,
                             float* __restrict__ out_dist,
                             int64_t* __restrict__ out_ids) {
  int64_t q = blockIdx.x;
  if (q >= nq) return;
  const float qn = (metric == 0 && add_qnorm) ? qnorms[q] : 0.f;
  for (int64_t i = lims[q] + threadIdx.x; i < lims[q + 1];
       i += blockDim.x) {
    uint64_t c = packed[i];
    uint32_t row = (uint32_t)c;
    out_dist[i] = range_dist(dec_f32((uint32_t)(c >> 32)), metric, add_qnorm,
                             qn);
    out_ids[i] = ids_lookup ? ids_lookup[row] : (int64_t)row;
  }
}

// ---------- misc small kernels ----------
__global__ void k_gather_rows_by_index(const float* __restrict__ src,
                                       const int64_t* __restrict__ idx,
                                       int64_t n, int32_t d,
                                       float* __restrict__ dst) {
  // dst[i] = src[idx[i]]  (wave per row)
  int64_t i = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  if (i >= n) return;
  if (d & 3) {  // PQ subspaces of dsub % 4 != 0: rows are not 16 B aligned
    const float* s1 = src + (size_t)idx[i] * d;
    float* t1 = dst + (size_t)i * d;
    for (int j = lane; j < d; j += WAVE) t1[j] = s1[j];
    return;
  }
  const float4* s = (const float4*)(src + (size_t)idx[i] * d);
  float4* t = (float4*)(dst + (size_t)i * d);
  for (int j = lane; j < d / 4; j += WAVE) t[j] = s[j];
}

__global__ void k_fill_base_total(int64_t nq, int64_t len, int64_t* base,
                                  int64_t* total) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  base[q] = q * len;
  total[q] = len;
}

__global__ void k_tombstone(const int64_t* __restrict__ pos, int64_t n,
                            int64_t* __restrict__ ids) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ids[pos[i]] = -2;
}

// ---------- columnar scan (v2) ----------
// The dominant kernel, redesigned: CSR chunks are stored TRANSPOSED
// ([d][nrows_pad] per 1024-row chunk).  Each lane owns
// 4 consecutive rows and accumulates full dots for QTM LDS-staged queries
// in registers — no cross-lane reduction at all (the v1 wave-per-row form
// was bound by its 6-deep dependent shuffle chain per (row, query)).
// Column loads are 16 B/lane coalesced; query element broadcasts come from
// LDS.  Unused query slots are zero-staged so the inner loop is branch-free.
template <int QTM, int RPL, bool NT = false>  // queries/tile, rows/lane
__device__ __forceinline__ void ivf_scan_col_body(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [QTM * d]
  int64_t* cbase = (int64_t*)(smem + (size_t)QTM * d);  // [QTM]

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  __builtin_assume(d % 4 == 0 && d > 0);  // host enforces; enables b128 LDS

  for (int32_t t0 = 0; t0 < nql; t0 += QTM) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    for (int32_t j = 0; j < qt; j++) {
      int32_t q = inv_q[iq0 + t0 + j];
      const float4* src = (const float4*)(queries + (size_t)q * d);
      float4* dst = (float4*)(smem + (size_t)j * d);
      for (int i = threadIdx.x; i < d / 4; i += blockDim.x) dst[i] = src[i];
    }
    // zero-stage unused slots (keeps the inner loop branch-free)
    for (size_t i = (size_t)qt * d + threadIdx.x; i < (size_t)QTM * d;
         i += blockDim.x)
      smem[i] = 0.f;
    if (threadIdx.x < QTM) {
      int32_t j = threadIdx.x;
      if (j < qt) {
        int32_t q = inv_q[iq0 + t0 + j];
        int32_t rank = inv_rank[iq0 + t0 + j];
        cbase[j] = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] -
                   list_start;
      } else {
        cbase[j] = 0;
      }
    }
    __syncthreads();

    // each wave covers WAVE*RPL consecutive rows; waves stride the chunk
    for (int32_t rb = wave_id * WAVE * RPL; rb < nrows_pad;
         rb += 4 * WAVE * RPL) {
      const int32_t rr0 = rb + lane * RPL;  // this lane's RPL rows
      if (rr0 >= nrows_pad) continue;
      float acc[QTM][RPL];
#pragma unroll
      for (int j = 0; j < QTM; j++)
#pragma unroll
        for (int x = 0; x < RPL; x++) acc[j][x] = 0.f;

      // dim loop unrolled by U, software-pipelined: while block i computes,
      // block i+U's loads are in flight (double-buffered column registers —
      // waiting within the issuing iteration exposes full HBM latency).
      // Query elements read 4-at-a-time from aligned LDS.
      constexpr int U = 4;
      static_assert(RPL == 1 || RPL == 2 || RPL % 4 == 0, "RPL");
      float ca[U][RPL], cb[U][RPL];
      const float* colp = col + rr0;
      auto load_block = [&](float (&c)[U][RPL], int32_t ib) {
#pragma unroll
        for (int u = 0; u < U; u++) {
          const float* cp = colp + (size_t)(ib + u) * nrows_pad;
          if (RPL >= 4) {
#pragma unroll
            for (int v = 0; v < RPL / 4; v++) {
              // nt (stream-once) column loads selectable: each chunk is
              // read by exactly one CU per batch, so L1/L2 retention buys
              // nothing (MI355X_MICROARCH.md nt-weights row)
              typedef float nf4 __attribute__((ext_vector_type(4)));
              float4 c4;
              if (NT) {
                const nf4 nv =
                    __builtin_nontemporal_load((const nf4*)cp + v);
                c4 = make_float4(nv[0], nv[1], nv[2], nv[3]);
              } else {
                c4 = ((const float4*)cp)[v];
              }
              c[u][4 * v + 0] = c4.x;
              c[u][4 * v + 1] = c4.y;
              c[u][4 * v + 2] = c4.z;
              c[u][4 * v + 3] = c4.w;
            }
          } else if (RPL == 2) {
            const float2 c2 = *(const float2*)cp;
            c[u][0] = c2.x; c[u][RPL - 1] = c2.y;
          } else {
            c[u][0] = *cp;
          }
        }
      };
      static_assert(U % 4 == 0, "U");
      auto compute_block = [&](float (&c)[U][RPL], int32_t ib) {
#pragma unroll
        for (int j = 0; j < QTM; j++) {
#pragma unroll
          for (int u4 = 0; u4 < U / 4; u4++) {
            // two b64 LDS reads (2cy/8B) instead of a float4 that lowers
            // to ds_read2_b32 (4cy/8B)
            const float* qp = smem + (size_t)j * d + ib + u4 * 4;
            const float2 qa = *(const float2*)qp;
            const float2 qb = *(const float2*)(qp + 2);
            const float qv[4] = {qa.x, qa.y, qb.x, qb.y};
#pragma unroll
            for (int uu = 0; uu < 4; uu++)
#pragma unroll
              for (int x = 0; x < RPL; x++)
                acc[j][x] += c[u4 * 4 + uu][x] * qv[uu];
          }
        }
      };
      // 2-deep rotation (3-deep costs a wave of occupancy and regresses)
      load_block(ca, 0);
      int32_t ib = 0;
      for (; ib + U < d; ib += 2 * U) {
        load_block(cb, ib + U);
        compute_block(ca, ib);
        if (ib + 2 * U < d) load_block(ca, ib + 2 * U);
        compute_block(cb, ib + U);
      }
      if (ib < d) compute_block(ca, ib);

      // emit: lane's rows are consecutive in each query's segment
      // (guards, not breaks: a break blocks full unroll and acc[] would be
      // dynamically indexed -> scratch spill)
#pragma unroll
      for (int j = 0; j < QTM; j++) {
        if (j < qt) {
          const int64_t cb = cbase[j] + row0 + rr0;
#pragma unroll
          for (int x = 0; x < RPL; x++) {
            const int32_t rl = rr0 + x;
            if (rl < nrows) {
              const int64_t r = row0 + rl;
              bool pass = true;
              if (bitmap) pass = (bitmap[r >> 5] >> (r & 31)) & 1;
              float key = (metric == 0) ? vnorms[r] - 2.0f * acc[j][x]
                                        : -acc[j][x];
              cand[cb + x] = pass ? pack_cand(key, (uint32_t)r) : kCandEmpty;
            }
          }
        }
      }
    }
  }
}

// ---------- IVF-PQ kernels ----------
// ADC decomposition: for L2,
//   ||q - (c_l + r)||^2 = ||q||^2 - 2*dots[q][l]
//                         + sum_m ( S[l][m][code] - 2*T[q][m][code] )
// with S[l][m][c] = ||centroid_l_sub_m + codebook_m[c]||^2 (index-static)
// and  T[q][m][c] = q_sub_m . codebook_m[c] (per batch, strided GEMM).
// For IP: score = dots[q][l] + sum_m T[q][m][code].
// Restates faiss IndexIVFPQ residual ADC (oracle.c dgo_ivfpq_search is the
// direct restatement; this is the same arithmetic regrouped).

__global__ void k_residual(const float* __restrict__ x,
                           const int32_t* __restrict__ assign,
                           const float* __restrict__ centroids, int64_t n,
                           int32_t d, float* __restrict__ out) {
  int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  if (row >= n) return;
  const float* v = x + (size_t)row * d;
  const float* c = centroids + (size_t)assign[row] * d;
  float* o = out + (size_t)row * d;
  for (int i = lane; i < d; i += WAVE) o[i] = v[i] - c[i];
}

// cs = bytes per code row.  nbits = 4 (faiss generic PQ packing): sub-
// quantizer 2j is the low nibble of byte j and 2j+1 the high one; even m
// stores the byte, odd m ORs into it, so the neighbour survives as long as
// the launches run in ascending m on one stream (pq_encode does).
__global__ void k_set_code(const int32_t* __restrict__ amin, int64_t n,
                           int32_t m, int32_t cs, int32_t nbits,
                           uint8_t* __restrict__ codes) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (nbits == 8) {
    codes[(size_t)i * cs + m] = (uint8_t)amin[i];
  } else {
    uint8_t* b = codes + (size_t)i * cs + (m >> 1);
    const uint8_t c = (uint8_t)(amin[i] & 15);
    *b = (m & 1) ? (uint8_t)(*b | (c << 4)) : c;
  }
}

__global__ void k_gather_codes(const uint8_t* __restrict__ src,
                               const uint32_t* __restrict__ perm, int64_t n,
                               int32_t M, uint8_t* __restrict__ dst) {
  // dst[perm[i]] = src[i], M bytes per row, dword copies
  int64_t i = (int64_t)blockIdx.x * (blockDim.x / 32) + threadIdx.x / 32;
  int sub = threadIdx.x % 32;
  if (i >= n) return;
  const uint32_t* s = (const uint32_t*)(src + (size_t)i * M);
  uint32_t* t = (uint32_t*)(dst + (size_t)perm[i] * M);
  for (int j = sub; j < M / 4; j += 32) t[j] = s[j];
}

static constexpr float kHalfMax = 65504.0f;  // largest finite f16

__global__ void k_build_S(const float* __restrict__ centroids,
                          const float* __restrict__ codebooks, int32_t nlist,
                          int32_t M, int32_t ksub, int32_t dsub, int32_t d,
                          __half* __restrict__ S,
                          int32_t* __restrict__ overflow) {
  // one thread per (l, m, code): ||c_sub + cb||^2 over dsub elems
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)nlist * M * ksub;
  if (i >= total) return;
  int32_t code = (int32_t)(i % ksub);
  int32_t m = (int32_t)((i / ksub) % M);
  int32_t l = (int32_t)(i / ((int64_t)ksub * M));
  const float* c = centroids + (size_t)l * d + m * dsub;
  const float* cb = codebooks + ((size_t)m * ksub + code) * dsub;
  float acc = 0.f;
  for (int32_t j = 0; j < dsub; j++) {
    float t = c[j] + cb[j];
    acc += t * t;
  }
  // an entry f16 cannot hold (it would round to inf, or is NaN already)
  // poisons every key of its list: raise the flag the host reads back
  if (!(acc <= kHalfMax)) atomicOr(overflow, 1);
  S[i] = __float2half(acc);
}

__global__ void k_f32_to_f16(const float* __restrict__ in, int64_t n,
                             __half* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = __float2half(in[i]);
}

// THE PQ scan: unit = (list, chunk of codes).  Codes for a RPV*64-vector tile
// are LDS-staged once and reused by every probing query; each LANE owns one
// vector and walks m = 0..M-1 sequentially, so all lanes of a wave gather
// within the same 1 KB rows of T[q] and S[l] (L1-resident after first
// touch).  No cross-lane reduction.
// COOP: all 4 waves walk the SAME query over disjoint quarters of the
// staged tile (one coherent 48 KB T-window in L1 at a time) instead of 4
// different queries (4 windows thrash the 32 KB L1).
template <int RPV, int MINB = 1, bool COOP = false>
__global__ void __launch_bounds__(256, MINB) k_ivfpq_scan(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const uint8_t* __restrict__ csr_codes, const __half* __restrict__ S,
    const __half* __restrict__ T, const float* __restrict__ coarse_dots,
    int32_t nlist, int32_t M, const int32_t* __restrict__ inv_offsets,
    const int32_t* __restrict__ inv_q, const int32_t* __restrict__ inv_rank,
    const int64_t* __restrict__ qp_off, const int64_t* __restrict__ q_cand_base,
    int32_t nprobe, int metric, const uint32_t* __restrict__ bitmap,
    int32_t chunk_rows, uint64_t* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_codes[];
  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t list_end = csr_offsets[list + 1];
  const int64_t row_start = list_start + (int64_t)chunk * chunk_rows;
  const int64_t row_end = min(list_end, row_start + chunk_rows);
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;
  if (nql == 0) return;  // unprobed list (all-chunks launch)
  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int32_t TILE = RPV * WAVE;  // vectors staged per pass

  // stage S_l into LDS once per unit (M*256 f16 = 48 KB at M=96); without
  // this every (wave, query, m) visit re-fetches a 512 B row from L2/HBM -
  // S exceeds L3 at cfg D and those fetches were the kernel's bound
  __half* lds_S = (__half*)(lds_codes + (size_t)TILE * M);
  {
    const uint32_t* src_s = (const uint32_t*)(S + (size_t)list * M * 256);
    uint32_t* dst_s = (uint32_t*)lds_S;
    const int32_t words = M * 256 / 2;
    for (int32_t w = threadIdx.x; w < words; w += blockDim.x)
      dst_s[w] = src_s[w];
  }
  __syncthreads();
  const __half* Sl = lds_S;

  for (int64_t t0 = row_start; t0 < row_end; t0 += TILE) {
    const int32_t tn = (int32_t)min((int64_t)TILE, row_end - t0);
    __syncthreads();
    {  // stage codes coalesced (rows are contiguous in csr_codes)
      const uint32_t* src = (const uint32_t*)(csr_codes + (size_t)t0 * M);
      uint32_t* dst = (uint32_t*)lds_codes;
      int32_t words = tn * M / 4;
      for (int32_t w = threadIdx.x; w < words; w += blockDim.x)
        dst[w] = src[w];
    }
    __syncthreads();

    // waves split the probing queries; each LANE owns RPV of the staged
    // vectors, so every (wave, query, m) visit of a 1 KB table row is
    // consumed by the whole tile — without this, 3 KB of S/T row traffic
    // per (vector, query) pair is the bottleneck (S at cfg D is 1.6 GB,
    // beyond L3).  COOP instead walks queries jointly (see above).
    constexpr int RV = COOP ? RPV / 4 : RPV;
    const int32_t vbase = COOP ? wave_id * (TILE / 4) : 0;
    for (int32_t qi = COOP ? 0 : wave_id; qi < nql;
         qi += COOP ? 1 : blockDim.x / WAVE) {
      const int32_t q = inv_q[iq0 + qi];
      const int32_t rank = inv_rank[iq0 + qi];
      const __half* Tq = T + (size_t)q * M * 256;
      const float dot = coarse_dots[(size_t)q * nlist + list];
      const int64_t cb0 = q_cand_base[q] +
                          qp_off[(int64_t)q * nprobe + rank] - list_start;
      float acc[RV];
      const uint32_t* code4[RV];
#pragma unroll
      for (int r = 0; r < RV; r++) {
        acc[r] = 0.f;
        code4[r] = (const uint32_t*)(lds_codes +
                                     (size_t)(vbase + lane + r * WAVE) * M);
      }
      if (metric == 0) {
        const __half* Sm = Sl;
        const __half* Tm = Tq;
        for (int32_t m4 = 0; m4 < M / 4; m4++) {
#pragma unroll
          for (int r = 0; r < RV; r++) {
            const uint32_t cw = code4[r][m4];
            const uint32_t c0 = cw & 255, c1 = (cw >> 8) & 255,
                           c2 = (cw >> 16) & 255, c3 = cw >> 24;
            acc[r] += (__half2float(Sm[c0]) + __half2float(Sm[256 + c1]) +
                       __half2float(Sm[512 + c2]) +
                       __half2float(Sm[768 + c3])) -
                      2.0f * (__half2float(Tm[c0]) +
                              __half2float(Tm[256 + c1]) +
                              __half2float(Tm[512 + c2]) +
                              __half2float(Tm[768 + c3]));
          }
          Sm += 1024;
          Tm += 1024;
        }
#pragma unroll
        for (int r = 0; r < RV; r++) acc[r] -= 2.0f * dot;  // +qnorm@emit
      } else {
        const __half* Tm = Tq;
        for (int32_t m4 = 0; m4 < M / 4; m4++) {
#pragma unroll
          for (int r = 0; r < RV; r++) {
            const uint32_t cw = code4[r][m4];
            acc[r] += __half2float(Tm[cw & 255]) +
                      __half2float(Tm[256 + ((cw >> 8) & 255)]) +
                      __half2float(Tm[512 + ((cw >> 16) & 255)]) +
                      __half2float(Tm[768 + (cw >> 24)]);
          }
          Tm += 1024;
        }
#pragma unroll
        for (int r = 0; r < RV; r++) acc[r] = -(acc[r] + dot);
      }
#pragma unroll
      for (int r = 0; r < RV; r++) {
        const int32_t v = vbase + lane + r * WAVE;
        if (v < tn) {
          const int64_t rw = t0 + v;
          bool pass = true;
          if (bitmap) pass = (bitmap[rw >> 5] >> (rw & 31)) & 1;
          cand[cb0 + rw] =
              pass ? pack_cand(acc[r], (uint32_t)rw) : kCandEmpty;
        }
      }
    }
  }
}

// THE 4-bit PQ scan (nbits = 4): unit structure, candidate layout and
// arguments of k_ivfpq_scan; S and T rows have 16 entries, csr_codes rows are
// M/2 packed bytes (sub-quantizer 2j in the low nibble of byte j), M % 8 == 0.
// Everything a lookup touches lives in LDS:
//   U[4 waves][M][16] f32 | S_l[M][16] f16 | codes[256 rows][stride dwords]
// Per (wave, query) the wave folds U[m][c] = S_l[m][c] - 2*T_q[m][c] (L2) or
// U = T_q (IP/cosine) and then walks the staged tile: each lane owns 4 rows,
// reads a row's codes one dword (8 sub-quantizers) at a time and adds
// U[m][nibble].  Bank argument: all lanes of a wave read
// the same 16-dword row of U at a time, 16 consecutive banks, equal addresses
// broadcast; the code row stride is odd, so the 32 lanes of a half wave read
// their row's dword w from 32 distinct banks.
__host__ __device__ static inline int32_t pq4_row_stride(int32_t M) {
  return (M / 8) | 1;  // dwords; odd
}

__global__ void __launch_bounds__(256) k_ivfpq4_scan(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const uint8_t* __restrict__ csr_codes, const __half* __restrict__ S,
    const __half* __restrict__ T, const float* __restrict__ coarse_dots,
    int32_t nlist, int32_t M, const int32_t* __restrict__ inv_offsets,
    const int32_t* __restrict__ inv_q, const int32_t* __restrict__ inv_rank,
    const int64_t* __restrict__ qp_off, const int64_t* __restrict__ q_cand_base,
    int32_t nprobe, int metric, const uint32_t* __restrict__ bitmap,
    int32_t chunk_rows, uint64_t* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds4[];
  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t list_end = csr_offsets[list + 1];
  const int64_t row_start = list_start + (int64_t)chunk * chunk_rows;
  const int64_t row_end = min(list_end, row_start + chunk_rows);
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;
  if (nql == 0) return;  // unprobed list (all-chunks launch)
  constexpr int NW = 4;              // waves per block
  constexpr int RV = 4;              // rows per lane
  constexpr int32_t TILE = RV * WAVE;  // == kPqTileRows
  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int32_t cw = M / 8;                // dwords of a packed code row
  const int32_t sw = pq4_row_stride(M);    // its LDS stride
  const int32_t tab = M * 16;              // entries of one table

  float* U = (float*)lds4 + (size_t)wave_id * tab;
  __half* Sl = (__half*)(lds4 + (size_t)NW * tab * 4);
  uint32_t* codes = (uint32_t*)(lds4 + (size_t)NW * tab * 4 + (size_t)tab * 2);

  {  // stage S_l once per unit (32*M bytes)
    const uint32_t* src_s = (const uint32_t*)(S + (size_t)list * tab);
    uint32_t* dst_s = (uint32_t*)Sl;
    for (int32_t w = threadIdx.x; w < tab / 2; w += blockDim.x)
      dst_s[w] = src_s[w];
  }

  for (int64_t t0 = row_start; t0 < row_end; t0 += TILE) {
    const int32_t tn = (int32_t)min((int64_t)TILE, row_end - t0);
    __syncthreads();  // the previous tile's readers are done
    {  // stage the packed rows, coalesced in, odd stride out
      const uint32_t* src =
          (const uint32_t*)(csr_codes + (size_t)t0 * cw * 4);
      const int32_t words = tn * cw;
      for (int32_t w = threadIdx.x; w < words; w += blockDim.x) {
        const int32_t r = w / cw;
        codes[r * sw + (w - r * cw)] = src[w];
      }
    }
    // every wave takes every trip (the barriers are block-wide); a wave
    // past the last probing query idles through them
    for (int32_t qb = 0; qb < nql; qb += NW) {
      const int32_t qi = qb + wave_id;
      const bool active = qi < nql;
      int32_t q = 0, rank = 0;
      __syncthreads();  // codes (and S_l) staged; last trip's U consumed
      if (active) {
        q = inv_q[iq0 + qi];
        rank = inv_rank[iq0 + qi];
        // fold the wave's table, 8 entries per lane and step
        const uint4* T8 = (const uint4*)(T + (size_t)q * tab);
        const uint4* S8 = (const uint4*)Sl;
        for (int32_t i = lane; i < tab / 8; i += WAVE) {
          const uint4 tv = T8[i];
          const uint32_t tw[4] = {tv.x, tv.y, tv.z, tv.w};
          float u[8];
          if (metric == 0) {
            const uint4 sv = S8[i];
            const uint32_t sx[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
              u[2 * j] = __half2float(__ushort_as_half(sx[j] & 0xffff)) -
                         2.0f * __half2float(__ushort_as_half(tw[j] & 0xffff));
              u[2 * j + 1] = __half2float(__ushort_as_half(sx[j] >> 16)) -
                             2.0f * __half2float(__ushort_as_half(tw[j] >> 16));
            }
          } else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
              u[2 * j] = __half2float(__ushort_as_half(tw[j] & 0xffff));
              u[2 * j + 1] = __half2float(__ushort_as_half(tw[j] >> 16));
            }
          }
          float4* dst = (float4*)(U + (size_t)i * 8);
          dst[0] = make_float4(u[0], u[1], u[2], u[3]);
          dst[1] = make_float4(u[4], u[5], u[6], u[7]);
        }
      }
      __syncthreads();  // U complete
      if (!active) continue;
      const float dot = coarse_dots[(size_t)q * nlist + list];
      const int64_t cb0 = q_cand_base[q] +
                          qp_off[(int64_t)q * nprobe + rank] - list_start;
      float acc[RV];
      const uint32_t* crow[RV];
#pragma unroll
      for (int r = 0; r < RV; r++) {
        acc[r] = 0.f;
        crow[r] = codes + (size_t)(lane + r * WAVE) * sw;
      }
      const float* Um = U;
      for (int32_t w = 0; w < cw; w++) {
#pragma unroll
        for (int r = 0; r < RV; r++) {
          const uint32_t c8 = crow[r][w];
#pragma unroll
          for (int j = 0; j < 8; j++)
            acc[r] += Um[j * 16 + ((c8 >> (4 * j)) & 15)];
        }
        Um += 128;
      }
#pragma unroll
      for (int r = 0; r < RV; r++) {
        const int32_t v = lane + r * WAVE;
        if (v < tn) {
          const int64_t rw = t0 + v;
          // L2: + ||q||^2 at emit; IP and cosine: larger is better
          const float key = metric == 0 ? acc[r] - 2.0f * dot
                                        : -(acc[r] + dot);
          bool pass = true;
          if (bitmap) pass = (bitmap[rw >> 5] >> (rw & 31)) & 1;
          cand[cb0 + rw] = pass ? pack_cand(key, (uint32_t)rw) : kCandEmpty;
        }
      }
    }
  }
}

// ---------- asm-pipelined columnar scan (v3, DG_SCAN_VARIANT=10) ----------
// Round-2 redesign of the dim loop.  The C++ double-buffer rotation of v2
// compiles to a register-allocator artifact: hipcc copies each loaded
// float4 into the loop-carried phi registers THROUGH an s_waitcnt vmcnt(0)
// placed right after the first load of the next block — the "pipeline"
// waits for the load it just issued, exposing full HBM latency (~900 cy)
// every 8 dims.  Here the loads are inline-asm global_load_dwordx4 into
// explicitly tied buffers with counted s_waitcnt vmcnt(N) (the compiler
// does not know the loads are pending, so it cannot insert its own waits),
// modulo-scheduled over DEPTH=4 stages x U=4 dims: 16 column loads stay in
// flight per lane while one stage computes — outstanding bytes per CU
// (8 waves x ~12 KB) far exceed the ~7 KB Little's-law need at the 6.3 TB/s
// achievable ceiling.  vmcnt discipline: the dim loop contains NO other
// vmem (a vmcnt(0) drain precedes the prologue so emit-stores of the
// previous tile don't skew the counts); loads past d land in d_csr_t's
// one-chunk slack and are never consumed.
typedef float dg_f4 __attribute__((ext_vector_type(4)));

// NOTE: the address must be bound as uint64_t — a pointer-typed "v"
// operand binds a single 32-bit VGPR and truncates the VA (measured: GPU
// memory fault at the truncated low-32-bit address).  "=&v" (early
// clobber) keeps the allocator from overlapping the destination tuple
// with the address pair: the hardware does not interlock VALU writes to
// an ASYNC load's destination, and the compiler cannot see that the asm
// load is still in flight.
#define DG_GLOAD4(dst, ptr)                                         \
  asm volatile("global_load_dwordx4 %0, %1, off"                    \
               : "=&v"(dst)                                         \
               : "v"((uint64_t)(uintptr_t)(ptr)))
// counted wait, tying the stage's 4 buffers so their consumers cannot be
// scheduled above the wait.  SAFE mode drains everything (diagnostic
// baseline for the counted schedule).
#define DG_WAITV(n, b)                                              \
  asm volatile("s_waitcnt vmcnt(" #n ")"                            \
               : "+v"((b)[0]), "+v"((b)[1]), "+v"((b)[2]), "+v"((b)[3]))
#define DG_WAITV_N(n, b)                                            \
  do {                                                              \
    if (SAFE)                                                       \
      DG_WAITV(0, b);                                               \
    else                                                            \
      DG_WAITV(n, b);                                               \
  } while (0)

// ---------- fused per-wave top-k epilogue (IVF-Flat top-k path) ----------
// Instead of storing every candidate and re-reading all of them in
// k_select_u64, the scan keeps only each wave's kf smallest candidates per
// staged query.  The top-k of a union is the top-k of the per-subset
// top-k's and packed candidates are unique per query (row in the low 32
// bits), so the later merge over the partial slots is bit-identical to a
// select over all candidates.

// min over the 64 lanes, returned wave-uniform.  DPP ladder: two quad
// permutes, half-mirror, mirror (each 16-lane row now uniform), then the
// gfx9 row broadcasts fold the four rows into lane 63.  Needs the whole
// wave converged.  Rows masked out of a step read the min identity (~0),
// which also lets the compiler fold each step into one v_min_u32_dpp.
__device__ __forceinline__ uint32_t dg_wave_min_u32(uint32_t v) {
#define DG_DPP(ctrl, rows)                                                 \
  ((uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, (ctrl), (rows), 0xf, \
                                         false))
  v = min(v, DG_DPP(0xB1, 0xf));   // quad_perm [1,0,3,2]
  v = min(v, DG_DPP(0x4E, 0xf));   // quad_perm [2,3,0,1]
  v = min(v, DG_DPP(0x141, 0xf));  // row_half_mirror
  v = min(v, DG_DPP(0x140, 0xf));  // row_mirror
  v = min(v, DG_DPP(0x142, 0xa));  // row_bcast15 into rows 1,3
  v = min(v, DG_DPP(0x143, 0xc));  // row_bcast31 into rows 2,3
#undef DG_DPP
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Select the wave's kf (<= 64) smallest candidates of each staged query
// from the lane's 4 accumulators and write them, ascending, to
// partial[cbase[j] + wslot .. + kf); unused tail entries are kCandEmpty.
// Extract-min on the 32-bit key; among equal keys the lowest lane, then the
// lowest x wins, which is the smaller row — the u64 order.  The one key
// value that a real candidate shares with kCandEmpty (0xffffffff, a NaN
// encoding) takes a plain u64 extract-min instead.
// Must be entered by ALL 64 lanes; lanes without rows pass rr0 >= nrows.
template <int JT>
__device__ __forceinline__ void dg_scan_topk_epilogue(
    const float (&acc)[JT][4], const int64_t* cbase, int64_t wslot,
    const float* __restrict__ vnorms, int32_t nrows, int32_t rr0,
    int64_t row0, int32_t qt, int metric, const uint32_t* __restrict__ bitmap,
    int32_t kf, uint64_t* __restrict__ partial) {
  constexpr int RPL = 4;
  const int lane = threadIdx.x % WAVE;
  const uint32_t rlo = (uint32_t)(row0 + rr0);
  bool ok[RPL];
  float vn[RPL];
#pragma unroll
  for (int x = 0; x < RPL; x++) {
    ok[x] = rr0 + x < nrows;
    vn[x] = 0.f;
    if (ok[x]) {
      const int64_t r = row0 + rr0 + x;
      if (bitmap) ok[x] = (bitmap[r >> 5] >> (r & 31)) & 1;
      if (metric == 0) vn[x] = vnorms[r];
    }
  }
#pragma unroll
  for (int j = 0; j < JT; j++) {
    if (j < qt) {
      uint32_t kx[RPL];
      bool odd = false;
#pragma unroll
      for (int x = 0; x < RPL; x++) {
        float key = (metric == 0) ? vn[x] - 2.0f * acc[j][x] : -acc[j][x];
        const uint32_t e = enc_f32(key);
        odd |= ok[x] && e == 0xffffffffu;
        kx[x] = ok[x] ? e : 0xffffffffu;
      }
      uint32_t res_hi = 0xffffffffu, res_lo = 0xffffffffu;
      if (__ballot(odd) == 0) {
        for (int32_t rnd = 0; rnd < kf; rnd++) {
          const uint32_t m = min(min(kx[0], kx[1]), min(kx[2], kx[3]));
          const uint32_t wm = dg_wave_min_u32(m);
          if (wm == 0xffffffffu) break;  // only empties left
          const int L = __builtin_ctzll(__ballot(m == wm));
          const uint32_t c =
              kx[0] == wm ? 0u : kx[1] == wm ? 1u : kx[2] == wm ? 2u : 3u;
          const uint32_t row =
              (uint32_t)__builtin_amdgcn_readlane((int)(rlo + c), L);
          const uint32_t sel = (lane == L) ? c : (uint32_t)RPL;
#pragma unroll
          for (int x = 0; x < RPL; x++)
            kx[x] = (sel == (uint32_t)x) ? 0xffffffffu : kx[x];
          if (lane == rnd) {
            res_hi = wm;
            res_lo = row;
          }
        }
      } else {
        uint64_t cv[RPL];
#pragma unroll
        for (int x = 0; x < RPL; x++)
          cv[x] = ok[x] ? (((uint64_t)kx[x] << 32) | (rlo + (uint32_t)x))
                        : kCandEmpty;
        for (int32_t rnd = 0; rnd < kf; rnd++) {
          uint64_t m = min(min(cv[0], cv[1]), min(cv[2], cv[3]));
          for (int off = 32; off; off >>= 1)
            m = min(m, (uint64_t)__shfl_xor((long long)m, off, WAVE));
          if (m == kCandEmpty) break;
#pragma unroll
          for (int x = 0; x < RPL; x++)
            if (cv[x] == m) cv[x] = kCandEmpty;
          if (lane == rnd) {
            res_hi = (uint32_t)(m >> 32);
            res_lo = (uint32_t)m;
          }
        }
      }
      if (lane < kf)
        partial[cbase[j] + wslot + lane] = ((uint64_t)res_hi << 32) | res_lo;
    }
  }
}

// row-scan body of k_ivf_scan_pipe, templated on the EFFECTIVE query-tile
// width JT: tiles that fill at most half the QTM slots take the JT=QTM/2
// instantiation and skip the zero-padded FMAs (at cfg C the mean tile
// holds ~8 of 16 queries — half the compute multiplies zeros otherwise).
// FUSED: every lane of the wave enters, rows or not, and the store of all
// candidates is replaced by dg_scan_topk_epilogue writing kf per wave at
// cbase[j] + wslot.
template <int JT, bool SAFE, bool FUSED = false>
__device__ __forceinline__ void dg_scan_rows_body(
    const float* smem, const int64_t* cbase, const float* col,
    const float* __restrict__ vnorms, int32_t d, int32_t nrows,
    int32_t nrows_pad, int32_t rr0, int64_t row0, int32_t qt, int metric,
    const uint32_t* __restrict__ bitmap, uint64_t* __restrict__ cand,
    int32_t kf = 0, int64_t wslot = 0) {
  constexpr int RPL = 4;
  constexpr int U = 4;
  float acc[JT][RPL];
#pragma unroll
  for (int j = 0; j < JT; j++)
#pragma unroll
    for (int x = 0; x < RPL; x++) acc[j][x] = 0.f;

  // drain prior vmem (previous tile's emit stores) so vmcnt counts below
  // track ONLY this loop's column loads
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // FUSED lanes past the chunk's rows re-read the chunk's first rows (no
  // new cache lines) and their sums are discarded by the epilogue
  const char* colp =
      (const char*)(col + ((!FUSED || rr0 < nrows_pad) ? rr0 : 0));
  const size_t cstride = (size_t)nrows_pad * 4;  // bytes per dim column
  dg_f4 b0[U], b1[U], b2[U], b3[U];
  auto issue = [&](dg_f4 (&b)[U], int32_t ib) {
    const char* p = colp + (size_t)ib * cstride;
#pragma unroll
    for (int u = 0; u < U; u++) DG_GLOAD4(b[u], p + u * cstride);
  };
  auto compute = [&](dg_f4 (&b)[U], int32_t ib) {
#pragma unroll
    for (int j = 0; j < JT; j++) {
      const float* qp = smem + (size_t)j * d + ib;
      const float2 qa = *(const float2*)qp;
      const float2 qb = *(const float2*)(qp + 2);
      const float qv[4] = {qa.x, qa.y, qb.x, qb.y};
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int x = 0; x < RPL; x++) acc[j][x] += b[u][x] * qv[u];
    }
  };
  // modulo schedule, period 4 stages = 16 dims
  issue(b0, 0);
  issue(b1, U);
  issue(b2, 2 * U);
  issue(b3, 3 * U);
  int32_t base = 0;
  for (; base + 16 < d; base += 16) {
    DG_WAITV_N(12, b0);
    compute(b0, base);
    issue(b0, base + 16);
    DG_WAITV_N(12, b1);
    compute(b1, base + 4);
    issue(b1, base + 20);
    DG_WAITV_N(12, b2);
    compute(b2, base + 8);
    issue(b2, base + 24);
    DG_WAITV_N(12, b3);
    compute(b3, base + 12);
    issue(b3, base + 28);
  }
  {  // epilogue: r = d - base in {4, 8, 12, 16} (d % 4 == 0)
    const int32_t r = d - base;
    DG_WAITV_N(12, b0);
    compute(b0, base);
    if (r > 4) {
      DG_WAITV_N(8, b1);
      compute(b1, base + 4);
    }
    if (r > 8) {
      DG_WAITV_N(4, b2);
      compute(b2, base + 8);
    }
    if (r > 12) {
      DG_WAITV(0, b3);
      compute(b3, base + 12);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  if (FUSED) {
    dg_scan_topk_epilogue<JT>(acc, cbase, wslot, vnorms, nrows, rr0, row0, qt,
                              metric, bitmap, kf, cand);
    return;
  }
#pragma unroll
  for (int j = 0; j < JT; j++) {
    if (j < qt) {
      const int64_t cb = cbase[j] + row0 + rr0;
#pragma unroll
      for (int x = 0; x < RPL; x++) {
        const int32_t rl = rr0 + x;
        if (rl < nrows) {
          const int64_t r = row0 + rl;
          bool pass = true;
          if (bitmap) pass = (bitmap[r >> 5] >> (r & 31)) & 1;
          float key = (metric == 0) ? vnorms[r] - 2.0f * acc[j][x]
                                    : -acc[j][x];
          cand[cb + x] = pass ? pack_cand(key, (uint32_t)r) : kCandEmpty;
        }
      }
    }
  }
}

// v6 (variant 19): two banks x 8 dims, ordered wait(A) -> issue(B_next)
// -> compute(A): the other bank's loads are issued a FULL 8-dim compute
// (~1000 cy) before their drain, so each drain should find them landed.
// Same full-drain tie discipline as the shipped pipeline.
template <int JT>
__device__ __forceinline__ void dg_scan_rows_body2(
    const float* smem, const int64_t* cbase, const float* col,
    const float* __restrict__ vnorms, int32_t d, int32_t nrows,
    int32_t nrows_pad, int32_t rr0, int64_t row0, int32_t qt, int metric,
    const uint32_t* __restrict__ bitmap, uint64_t* __restrict__ cand) {
  constexpr int RPL = 4;
  float acc[JT][RPL];
#pragma unroll
  for (int j = 0; j < JT; j++)
#pragma unroll
    for (int x = 0; x < RPL; x++) acc[j][x] = 0.f;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const char* colp = (const char*)(col + rr0);
  const size_t cstride = (size_t)nrows_pad * 4;
  dg_f4 A[8], B[8];
  auto issue8 = [&](dg_f4 (&b)[8], int32_t ib) {
#pragma unroll
    for (int u = 0; u < 8; u++)
      DG_GLOAD4(b[u], colp + (size_t)(ib + u) * cstride);
  };
  auto wait8 = [&](dg_f4 (&b)[8]) {
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]),
                   "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]));
  };
  auto compute8 = [&](dg_f4 (&b)[8], int32_t ib) {
#pragma unroll
    for (int j = 0; j < JT; j++) {
      const float* qp = smem + (size_t)j * d + ib;
#pragma unroll
      for (int h = 0; h < 4; h++) {
        const float2 qq = *(const float2*)(qp + 2 * h);
#pragma unroll
        for (int x = 0; x < RPL; x++)
          acc[j][x] += b[2 * h][x] * qq.x + b[2 * h + 1][x] * qq.y;
      }
    }
  };
  int32_t base = 0;
  if (d >= 16) {
    issue8(A, 0);
    for (; base + 16 <= d; base += 16) {
      wait8(A);
      if (base + 24 <= d) issue8(B, base + 8);
      compute8(A, base);
      if (base + 24 <= d) {
        wait8(B);
        if (base + 32 <= d) issue8(A, base + 16);
        compute8(B, base + 8);
      } else {
        // last 8 dims of the main region handled by the tail below
        base += 8;
        break;
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  const float* colf = col + rr0;
  for (int32_t ib = base; ib < d; ib += 4) {
    float4 c[4];
#pragma unroll
    for (int u = 0; u < 4; u++)
      c[u] = (ib + u < d)
                 ? *(const float4*)(colf + (size_t)(ib + u) * nrows_pad)
                 : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < JT; j++) {
      const float* qp = smem + (size_t)j * d + ib;
#pragma unroll
      for (int u = 0; u < 4 && ib + u < d; u++) {
        const float qv = qp[u];
        acc[j][0] += c[u].x * qv;
        acc[j][1] += c[u].y * qv;
        acc[j][2] += c[u].z * qv;
        acc[j][3] += c[u].w * qv;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int j = 0; j < JT; j++) {
    if (j < qt) {
      const int64_t cb = cbase[j] + row0 + rr0;
#pragma unroll
      for (int x = 0; x < RPL; x++) {
        const int32_t rl = rr0 + x;
        if (rl < nrows) {
          const int64_t r = row0 + rl;
          bool pass = true;
          if (bitmap) pass = (bitmap[r >> 5] >> (r & 31)) & 1;
          float key = (metric == 0) ? vnorms[r] - 2.0f * acc[j][x]
                                    : -acc[j][x];
          cand[cb + x] = pass ? pack_cand(key, (uint32_t)r) : kCandEmpty;
        }
      }
    }
  }
}

// FUSED (IVF-Flat top-k path): `cand` is the partial-slot buffer
//   [nq][nprobe][cpl_max][chunk_rows/256][kf]
// (cpl_max = chunks of the longest list); each wave writes its kf smallest
// per staged query, every (q, rank, chunk, wave) slot is written at most
// once and the host presets the buffer to kCandEmpty.  qp_off and
// q_cand_base are unused.
template <int QTM, bool SAFE = false, bool FUSED = false>
__global__ void __launch_bounds__(256, 1) k_ivf_scan_pipe(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand, int32_t kf = 0, int32_t cpl_max = 0) {
  constexpr int RPL = 4;  // rows per lane (float4 column loads)
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [QTM * d]
  int64_t* cbase = (int64_t*)(smem + (size_t)QTM * d);          // [QTM]

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  __builtin_assume(d % 4 == 0 && d > 0);

  for (int32_t t0 = 0; t0 < nql; t0 += QTM) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    for (int32_t j = 0; j < qt; j++) {
      int32_t q = inv_q[iq0 + t0 + j];
      const float4* src = (const float4*)(queries + (size_t)q * d);
      float4* dst = (float4*)(smem + (size_t)j * d);
      for (int i = threadIdx.x; i < d / 4; i += blockDim.x) dst[i] = src[i];
    }
    for (size_t i = (size_t)qt * d + threadIdx.x; i < (size_t)QTM * d;
         i += blockDim.x)
      smem[i] = 0.f;
    if (threadIdx.x < QTM) {
      int32_t j = threadIdx.x;
      if (j < qt) {
        int32_t q = inv_q[iq0 + t0 + j];
        int32_t rank = inv_rank[iq0 + t0 + j];
        if (FUSED)
          cbase[j] = ((((int64_t)q * nprobe + rank) * cpl_max + chunk) *
                      (chunk_rows / (WAVE * RPL))) * kf;
        else
          cbase[j] = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] -
                     list_start;
      } else {
        cbase[j] = 0;
      }
    }
    __syncthreads();

    // rb is wave-uniform: a wave either runs a row block whole (FUSED: all
    // 64 lanes, so the epilogue's cross-lane steps see a converged wave) or
    // skips it, leaving its slot at the preset kCandEmpty
    for (int32_t rb = wave_id * WAVE * RPL; rb < nrows_pad;
         rb += 4 * WAVE * RPL) {
      const int32_t rr0 = rb + lane * RPL;
      if (!FUSED && rr0 >= nrows_pad) continue;
      const int64_t wslot = (int64_t)(rb / (WAVE * RPL)) * kf;
      if (QTM >= 16 && qt <= QTM / 2)
        dg_scan_rows_body<(QTM >= 16 ? QTM / 2 : QTM), SAFE, FUSED>(
            smem, cbase, col, vnorms, d, nrows, nrows_pad, rr0, row0, qt,
            metric, bitmap, cand, kf, wslot);
      else
        dg_scan_rows_body<QTM, SAFE, FUSED>(smem, cbase, col, vnorms, d,
                                            nrows, nrows_pad, rr0, row0, qt,
                                            metric, bitmap, cand, kf, wslot);
    }
  }
}

// ---------- f32-MFMA fused top-k scan (IVF-Flat top-k default) ----------
// Same inputs, grid, query-tile loop and partial-slot output as
// k_ivf_scan_pipe<QTM,true,true>; the (row, query) dots come from
// v_mfma_f32_16x16x4_f32, whose result is a k-ordered fmaf chain with one
// rounding per product — the same bits as the VALU kernels' ascending-dim
// chain from 0.  For lane l, g = l>>4, i = l&15:
//   A (queries): lane (g,i) holds q_i[k0+g]
//   B (rows)   : one float4 per lane at col[(k0+g)*nrows_pad + rb+64m+4i],
//                m = 0..3; component x feeds tile (m,x), whose column i is
//                row rb+64m+4i+x
//   D          : lane (g,j), reg r = dot(query 4g+r, row rb+64m+4j+x)
// A k-step (4 dims) is 4 loads and 16 MFMAs into 16 independent
// accumulators.  The loads are plain C++ in a modulo-unrolled 4-stage loop
// (one named buffer set per stage), so the compiler tracks what is in
// flight and places its own counted waits; the sched_barrier keeps each
// stage's re-issue right behind that stage's MFMAs.
// Queries are staged permuted, [d/16][QTM][g 4][s 4] for dim 16kb+4s+g, so
// one ds_read_b128 gives a lane its A operands for four k-steps.
typedef float dg_acc4 __attribute__((ext_vector_type(4)));

// Lane id from mbcnt, seeded through an empty asm so that each use site
// computes it (and everything derived from it) afresh: with wave_id in an
// SGPR the kernel then holds no work-item id, and nothing computed from
// one, in registers across the dim loop (at 168 VGPRs that spills).
__device__ __forceinline__ int dg_lane_id_fresh() {
  uint32_t z = 0;
  asm volatile("" : "+v"(z));
  return (int)__builtin_amdgcn_mbcnt_hi(~0u,
                                        __builtin_amdgcn_mbcnt_lo(~0u, z));
}

// min over each 16-lane row (uniform within the row afterwards)
__device__ __forceinline__ uint32_t dg_row16_min_u32(uint32_t v) {
#define DG_DPP(ctrl)                                                      \
  ((uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, (ctrl), 0xf, 0xf,    \
                                         false))
  v = min(v, DG_DPP(0xB1));   // quad_perm [1,0,3,2]
  v = min(v, DG_DPP(0x4E));   // quad_perm [2,3,0,1]
  v = min(v, DG_DPP(0x141));  // row_half_mirror
  v = min(v, DG_DPP(0x140));  // row_mirror
#undef DG_DPP
  return v;
}

// Per-wave top-k for the MFMA register layout.  For a fixed reg r the four
// 16-lane rows hold four different queries (4g+r), each row's 16 lanes x 16
// tiles being that query's 256 rows, so one row-wise DPP ladder serves four
// queries per round.  Extract-min on the 32-bit key, then, among the live
// entries holding that key, on the chunk-local row (64m+4j+x is not
// monotone in lane order, so the tie needs its own min).  `live` rather
// than the key value marks what is still a candidate, so a real key that
// encodes as 0xffffffff still ranks by the u64 order.  The winner's lane
// stores slot `rnd`; the tail keeps the host's kCandEmpty preset.
// Must be entered by ALL 64 lanes.
__device__ __forceinline__ void dg_scan_topk_epilogue_mfma(
    const dg_acc4 (&acc)[4][4], const int64_t* cbase, int64_t wslot,
    const float* __restrict__ vnorms, int32_t nrows, int32_t rb, int64_t row0,
    int32_t qt, int metric, const uint32_t* __restrict__ bitmap, int32_t kf,
    uint64_t* __restrict__ partial) {
  const int lane = dg_lane_id_fresh();
  const int g = lane >> 4, j = lane & 15;
  // rows past the chunk read the chunk's last row (rb < nrows_pad, so
  // nrows >= 1) and are masked out: no per-entry branch
  bool okb[16];
  float vn[16];
  const float* vnb = vnorms + row0;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int32_t rl = rb + 64 * (e >> 2) + 4 * j + (e & 3);
    const int32_t rc = min(rl, nrows - 1);
    bool ok = rl < nrows;
    if (bitmap) {
      const int64_t r = row0 + rc;
      ok = ok && ((bitmap[r >> 5] >> (r & 31)) & 1);
    }
    vn[e] = (metric == 0) ? vnb[rc] : 0.f;
    okb[e] = ok;
  }
  uint32_t okm = 0;  // shifted in from the top: no per-bit constants
#pragma unroll
  for (int e = 15; e >= 0; e--) okm = (okm << 1) | (okb[e] ? 1u : 0u);
  const uint32_t rlo = (uint32_t)(row0 + rb);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (r >= qt) break;  // wave-uniform: no row of lanes has query 4g+r
    const int jq = 4 * g + r;
    const bool act = jq < qt;
    uint32_t live = act ? okm : 0u;
    const int64_t cb = act ? cbase[jq] + wslot : 0;
    uint32_t kx[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
      const float a = acc[e >> 2][e & 3][r];
      const float key = (metric == 0) ? vn[e] - 2.0f * a : -a;
      kx[e] = ((live >> e) & 1u) ? enc_f32(key) : 0xffffffffu;
    }
    for (int32_t rnd = 0; rnd < kf; rnd++) {
      uint32_t m = kx[0];
#pragma unroll
      for (int e = 1; e < 16; e++) m = min(m, kx[e]);
      const uint32_t wm = dg_row16_min_u32(m);
      uint32_t eq = 0;
#pragma unroll
      for (int e = 15; e >= 0; e--) eq = (eq << 1) | (kx[e] == wm ? 1u : 0u);
      eq &= live;
      // entries ascend in row within a lane, so the lowest set bit is the
      // lane's smallest row holding the key
      const uint32_t ce = eq ? (uint32_t)__builtin_ctz(eq) : 16u;
      const uint32_t ridx =
          eq ? (ce >> 2) * 64u + 4u * (uint32_t)j + (ce & 3u) : 0xffffffffu;
      const uint32_t wr = dg_row16_min_u32(ridx);
      if (__ballot(wr != 0xffffffffu) == 0) break;  // every query exhausted
      const bool win = ridx == wr && eq != 0;
      const uint32_t sel = win ? ce : 16u;
#pragma unroll
      for (int e = 0; e < 16; e++)
        kx[e] = (sel == (uint32_t)e) ? 0xffffffffu : kx[e];
      if (win) {
        live &= ~(1u << ce);
        partial[cb + rnd] = ((uint64_t)wm << 32) | (uint64_t)(rlo + wr);
      }
    }
  }
}

template <int QTM>
__global__ void __launch_bounds__(256, 3) k_ivf_scan_mfma(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ partial, int32_t kf, int32_t cpl_max,
    int32_t pairing) {
  static_assert(QTM <= 16 && QTM % 4 == 0, "one 16-query MFMA tile");
  // [nper][QTM][4][4] floats, then cbase[QTM]
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __builtin_assume(d % 4 == 0 && d > 0);
  const int32_t nks = d >> 2;          // k-steps of 4 dims
  const int32_t nper = (nks + 3) >> 2;  // periods of 4 k-steps
  int64_t* cbase = (int64_t*)(smem + (size_t)nper * QTM * 16);

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  // wave_id in an SGPR keeps rb and all it feeds scalar
  const int wave_id =
      __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  // bytes per k-step (4 columns); a chunk is at most 8192 x 1024 floats,
  // so 32 bits hold every byte offset into it
  const uint32_t kstepb = (uint32_t)nrows_pad * 16u;

  // with pairing on (QTM 16 only) k_ivf_scan_mfma2 has taken the list's
  // tile pairs: what is left is the odd last tile, or nothing
  for (int32_t t0 = kScanTileQ * dg_scan_single_first(nql, pairing != 0);
       t0 < nql; t0 += QTM) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    // float4 t of query j holds dims 4t..4t+3 = 16kb + 4s + g for g = 0..3
    // (kb = t>>2, s = t&3); absent queries and absent dims are zero
    const int tid = wave_id * WAVE + dg_lane_id_fresh();
#pragma unroll 1
    for (int32_t j = 0; j < QTM; j++) {
      const float4* src =
          j < qt ? (const float4*)(queries +
                                   (size_t)inv_q[iq0 + t0 + j] * d)
                 : nullptr;
      for (int32_t t = tid; t < nper * 4; t += blockDim.x) {
        float4 v = float4{0.f, 0.f, 0.f, 0.f};
        if (src && t < nks) v = src[t];
        float* dst = smem + ((size_t)(t >> 2) * QTM + j) * 16 + (t & 3);
        dst[0] = v.x;
        dst[4] = v.y;
        dst[8] = v.z;
        dst[12] = v.w;
      }
    }
    if (tid < QTM) {
      const int32_t j = tid;
      int64_t cb = 0;
      if (j < qt)
        cb = ((((int64_t)inv_q[iq0 + t0 + j] * nprobe +
                inv_rank[iq0 + t0 + j]) * cpl_max + chunk) *
              (chunk_rows / (WAVE * 4))) * kf;
      cbase[j] = cb;
    }
    __syncthreads();

    // rb is wave-uniform: a wave runs a 256-row block whole (all 64 lanes
    // reach the epilogue converged) or skips it, leaving its slots at the
    // preset kCandEmpty
    for (int32_t rb = wave_id * WAVE * 4; rb < nrows_pad; rb += 4 * WAVE * 4) {
      const int64_t wslot = (int64_t)(rb / (WAVE * 4)) * kf;
      const int lane = dg_lane_id_fresh();
      const int g = lane >> 4, i = lane & 15;
      // lanes past the chunk's rows re-read its first rows (no new cache
      // lines, nothing outside the chunk); the epilogue discards their sums
      // byte offsets from a wave-uniform column pointer: a chunk is at
      // most 8192 x 1024 floats, so 32 bits hold them
      uint32_t voff[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int32_t rr = rb + 64 * m + 4 * i;
        voff[m] = ((uint32_t)g * (uint32_t)nrows_pad +
                   (uint32_t)(rr < nrows_pad ? rr : 0)) * 4u;
      }
      const dg_acc4* ap = (const dg_acc4*)smem + (i < QTM ? i : 0) * 4 + g;

      // (zero through an empty asm: as a known constant the compiler keeps
      // a zero vector live across the dim loop and spills it)
      float z = 0.f;
      asm volatile("" : "+v"(z));
      dg_acc4 acc[4][4];
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int x = 0; x < 4; x++) acc[m][x] = dg_acc4{z, z, z, z};
      dg_acc4 b0[4], b1[4], b2[4], b3[4];
      auto issue = [&](dg_acc4 (&b)[4], int32_t ks) {
        // readfirstlane hides the k-step offset from loop strength
        // reduction (which would keep 16 per-lane 64-bit pointers and
        // spill) and pins it to an SGPR: scalar base + 32-bit lane offset
        const uint32_t uo =
            __builtin_amdgcn_readfirstlane((uint32_t)ks * kstepb);
#pragma unroll
        for (int m = 0; m < 4; m++)
          b[m] = *(const dg_acc4*)((const char*)col + (voff[m] + uo));
      };
      auto compute = [&](const dg_acc4 (&b)[4], float a) {
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
          for (int x = 0; x < 4; x++)
            acc[m][x] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a, b[m][x], acc[m][x], 0, 0, 0);
      };
      auto qload = [&]() {
        dg_acc4 a = *ap;
        ap += QTM * 4;
        if (QTM < 16 && i >= QTM) a = dg_acc4{0.f, 0.f, 0.f, 0.f};
        return a;
      };

      // modulo schedule, period = 4 stages = 16 dims; a stage is re-issued
      // for the next period as soon as its MFMAs are out
      // (the prologue issues all four stages in the loop's order so the
      // compiler's wait counts agree at the loop head; for d < 16 the
      // absent stages re-read the last column and are never consumed)
      issue(b0, 0);
      __builtin_amdgcn_sched_barrier(0);
      issue(b1, min(1, nks - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b2, min(2, nks - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b3, min(3, nks - 1));
      __builtin_amdgcn_sched_barrier(0);
      int32_t ks = 0;
      for (; ks + 8 <= nks; ks += 4) {  // the next period is whole too
        const dg_acc4 a = qload();
        compute(b0, a.x);
        __builtin_amdgcn_sched_barrier(0);
        issue(b0, ks + 4);
        compute(b1, a.y);
        __builtin_amdgcn_sched_barrier(0);
        issue(b1, ks + 5);
        compute(b2, a.z);
        __builtin_amdgcn_sched_barrier(0);
        issue(b2, ks + 6);
        compute(b3, a.w);
        __builtin_amdgcn_sched_barrier(0);
        issue(b3, ks + 7);
      }
      if (ks + 4 < nks) {  // whole period followed by a 1..3-step one
        const int32_t rem = nks - ks - 4;
        const dg_acc4 a = qload();
        compute(b0, a.x);
        __builtin_amdgcn_sched_barrier(0);
        issue(b0, ks + 4);
        compute(b1, a.y);
        __builtin_amdgcn_sched_barrier(0);
        if (rem > 1) issue(b1, ks + 5);
        compute(b2, a.z);
        __builtin_amdgcn_sched_barrier(0);
        if (rem > 2) issue(b2, ks + 6);
        compute(b3, a.w);
        ks += 4;
      }
      {  // last period: 1..4 k-steps; absent steps are skipped, not padded
        const int32_t rem = nks - ks;
        const dg_acc4 a = qload();
        compute(b0, a.x);
        if (rem > 1) compute(b1, a.y);
        if (rem > 2) compute(b2, a.z);
        if (rem > 3) compute(b3, a.w);
      }
      dg_scan_topk_epilogue_mfma(acc, cbase, wslot, vnorms, nrows, rb, row0,
                                 qt, metric, bitmap, kf, partial);
    }
  }
}

// ---------- f16 row storage (DG_STORAGE_F16) ----------
// Rows are stored as IEEE halves, the query stays f32.  k_ivf_scan_f16 is
// k_ivf_scan_mfma with the halves decoded in registers: the same 16x16x4 f32
// MFMA mapping, accumulator layout, row ownership and per-wave epilogue, so
// a distance is the f32 k-ordered chain over the f32 query and the decoded
// row (exact products: a half has 11 significant bits).
//
// Chunk layout, written by k_transpose_chunks_f16: with d8 = ceil(d/8)*8
// (dims past d are zeros) and nrows_pad = ceil(nrows/4)*4 (rows past nrows
// are zeros), a chunk is [d8/8 kp][4 g][nrows_pad/4 quads][2 h][4 x] halves
// holding dim 8kp + 4h + g of row 4*quad + x.  A lane's 16-byte load at
// ((4kp + g) * nrows_pad + row) * 4 bytes is the B operand (k = g) of the
// k-steps 2kp (h = 0) and 2kp+1 (h = 1) for four consecutive rows: the byte
// offsets are those of the f32 layout, each load feeding two k-steps.  A
// chunk is d8 * nrows_pad halves, a multiple of 64 bytes.  Every load falls
// inside the chunk (lanes past nrows_pad re-read its first quad, absent
// prologue stages re-read its last kp), so the buffer needs no slack.
typedef _Float16 dg_h8 __attribute__((ext_vector_type(8)));

__global__ void k_f32_to_f16_check(const float* __restrict__ in, int64_t n,
                                   __half* __restrict__ out,
                                   int32_t* __restrict__ overflow) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = in[i];
  if (!(fabsf(v) <= kHalfMax)) atomicOr(overflow, 1);  // NaN fails too
  out[i] = __float2half_rn(v);
}

__global__ void k_row_norms_f16(const __half* __restrict__ x, int64_t n,
                                int32_t d, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) +
                      threadIdx.x / WAVE;
  if (row >= n) return;
  const int lane = threadIdx.x % WAVE;
  const __half* p = x + (size_t)row * d;
  float s = 0.f;
  for (int32_t i = lane; i < d; i += WAVE) {
    const float v = __half2float(p[i]);
    s += v * v;
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (lane == 0) out[row] = s;
}

// out[i] = decoded row idx[i] of src, d_src halves per row, d floats out
__global__ void k_gather_rows_by_index_f16(const __half* __restrict__ src,
                                           const int64_t* __restrict__ idx,
                                           int64_t n, int32_t d,
                                           float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * d) return;
  const int64_t r = i / d;
  const int32_t c = (int32_t)(i - r * d);
  dst[i] = __half2float(src[(size_t)idx[r] * d + c]);
}

__global__ void __launch_bounds__(256) k_transpose_chunks_f16(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const __half* __restrict__ rowmajor, int32_t d, int32_t chunk_rows,
    __half* __restrict__ tvec) {
  __shared__ uint16_t tile[64][66];
  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const int32_t d8 = (d + 7) & ~7;
  const uint16_t* src = (const uint16_t*)rowmajor +
                        (list_start + (int64_t)chunk * chunk_rows) * d;
  uint16_t* dst =
      (uint16_t*)tvec + chunk_base[chunk_off[list] + (int32_t)chunk];

  const int tx = threadIdx.x % 64;
  const int ty = threadIdx.x / 64;
  for (int32_t r0 = 0; r0 < nrows_pad; r0 += 64) {
    for (int32_t i0 = 0; i0 < d8; i0 += 64) {
      __syncthreads();
      for (int rr = ty; rr < 64; rr += 4) {
        const int32_t r = r0 + rr;
        tile[rr][tx] = (r < nrows && i0 + tx < d)
                           ? src[(size_t)r * d + i0 + tx]
                           : (uint16_t)0;
      }
      __syncthreads();
      // 8 kp x 4 g x 16 quads = 512 16-byte groups per tile
      for (int t = threadIdx.x; t < 512; t += 256) {
        const int quad = t & 15, g = (t >> 4) & 3, kpl = t >> 6;
        const int32_t kp = (i0 >> 3) + kpl;
        const int32_t r = r0 + 4 * quad;
        if (8 * kp < d8 && r < nrows_pad) {
          uint32_t w[4];  // one 16-byte store: chunks are 64-byte aligned
#pragma unroll
          for (int h = 0; h < 2; h++)
#pragma unroll
            for (int x = 0; x < 4; x += 2)
              w[2 * h + (x >> 1)] =
                  (uint32_t)tile[4 * quad + x][8 * kpl + 4 * h + g] |
                  ((uint32_t)tile[4 * quad + x + 1][8 * kpl + 4 * h + g]
                   << 16);
          *(uint4*)(dst + ((size_t)(4 * kp + g) * nrows_pad + r) * 2) =
              make_uint4(w[0], w[1], w[2], w[3]);
        }
      }
    }
  }
}

// Store-all epilogue for the MFMA register layout: every (query, row) pair of
// the wave's 256-row block goes to the dense candidate buffer
// (cand[cbase[query] + chunk-local row], the layout of ivf_scan_col_body),
// with the key expression of dg_scan_topk_epilogue_mfma.
__device__ __forceinline__ void dg_scan_store_epilogue_mfma(
    const dg_acc4 (&acc)[4][4], const int64_t* cbase,
    const float* __restrict__ vnorms, int32_t nrows, int32_t rb, int64_t row0,
    int32_t qt, int metric, const uint32_t* __restrict__ bitmap,
    uint64_t* __restrict__ cand) {
  const int lane = dg_lane_id_fresh();
  const int g = lane >> 4, j = lane & 15;
#pragma unroll
  for (int e = 0; e < 16; e++) {
    const int32_t rl = rb + 64 * (e >> 2) + 4 * j + (e & 3);
    if (rl >= nrows) continue;
    const int64_t r = row0 + rl;
    bool pass = true;
    if (bitmap) pass = (bitmap[r >> 5] >> (r & 31)) & 1;
    const float vn = (metric == 0) ? vnorms[r] : 0.f;
#pragma unroll
    for (int rq = 0; rq < 4; rq++) {
      const int jq = 4 * g + rq;
      if (jq < qt) {
        const float a = acc[e >> 2][e & 3][rq];
        const float key = (metric == 0) ? vn - 2.0f * a : -a;
        cand[cbase[jq] + rl] = pass ? pack_cand(key, (uint32_t)r) : kCandEmpty;
      }
    }
  }
}

// FUSED: per-wave top-k into `out` (= partial, qp_off / q_cand_base unused);
// otherwise every candidate into `out` (= cand).  One dot-product body.
template <int QTM, bool FUSED>
__global__ void __launch_bounds__(256, 2) k_ivf_scan_f16(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const __half* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ out, int32_t kf, int32_t cpl_max) {
  static_assert(QTM <= 16 && QTM % 4 == 0, "one 16-query MFMA tile");
  // [nper][QTM][4][4] floats (nper even: whole 32-dim periods), cbase[QTM]
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __builtin_assume(d % 4 == 0 && d > 0);
  const int32_t nf4 = d >> 2;             // float4s of a query
  const int32_t nkp = (d + 7) >> 3;       // loads per lane and m: 8 dims each
  const int32_t nper = ((nkp + 3) >> 2) * 2;  // 16-dim LDS periods
  int64_t* cbase = (int64_t*)(smem + (size_t)nper * QTM * 16);

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const __half* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  const int wave_id =
      __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  // bytes per kp (8 dims x nrows_pad halves); a chunk is at most 8192 x 1024
  // halves, so 32 bits hold every byte offset into it
  const uint32_t kstepb = (uint32_t)nrows_pad * 16u;

  // a list's query tiles are strided over grid.y, so that a list probed by
  // many queries is not one block's serial work (DESIGN.md §f16 row
  // storage has the measurement); tiles are independent, the slots and
  // candidates of a query are written by its own tile alone
  for (int32_t t0 = QTM * (int32_t)blockIdx.y; t0 < nql;
       t0 += QTM * (int32_t)gridDim.y) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    // the LDS image of k_ivf_scan_mfma: float4 t of query j holds dims
    // 16kb + 4s + g (kb = t>>2, s = t&3); absent queries and dims are zero
    const int tid = wave_id * WAVE + dg_lane_id_fresh();
#pragma unroll 1
    for (int32_t j = 0; j < QTM; j++) {
      const float4* src =
          j < qt ? (const float4*)(queries +
                                   (size_t)inv_q[iq0 + t0 + j] * d)
                 : nullptr;
      for (int32_t t = tid; t < nper * 4; t += blockDim.x) {
        float4 v = float4{0.f, 0.f, 0.f, 0.f};
        if (src && t < nf4) v = src[t];
        float* dst = smem + ((size_t)(t >> 2) * QTM + j) * 16 + (t & 3);
        dst[0] = v.x;
        dst[4] = v.y;
        dst[8] = v.z;
        dst[12] = v.w;
      }
    }
    if (tid < QTM) {
      const int32_t j = tid;
      int64_t cb = 0;
      if (j < qt) {
        const int32_t q = inv_q[iq0 + t0 + j];
        const int32_t rank = inv_rank[iq0 + t0 + j];
        if (FUSED)
          cb = ((((int64_t)q * nprobe + rank) * cpl_max + chunk) *
                (chunk_rows / (WAVE * 4))) * kf;
        else
          cb = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] +
               (int64_t)chunk * chunk_rows;
      }
      cbase[j] = cb;
    }
    __syncthreads();

    for (int32_t rb = wave_id * WAVE * 4; rb < nrows_pad; rb += 4 * WAVE * 4) {
      const int lane = dg_lane_id_fresh();
      const int g = lane >> 4, i = lane & 15;
      uint32_t voff[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int32_t rr = rb + 64 * m + 4 * i;
        voff[m] = ((uint32_t)g * (uint32_t)nrows_pad +
                   (uint32_t)(rr < nrows_pad ? rr : 0)) * 4u;
      }
      const dg_acc4* ap = (const dg_acc4*)smem + (i < QTM ? i : 0) * 4 + g;

      float z = 0.f;
      asm volatile("" : "+v"(z));
      dg_acc4 acc[4][4];
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int x = 0; x < 4; x++) acc[m][x] = dg_acc4{z, z, z, z};
      dg_h8 b0[4], b1[4], b2[4], b3[4];
      auto issue = [&](dg_h8 (&b)[4], int32_t kp) {
        const uint32_t uo =
            __builtin_amdgcn_readfirstlane((uint32_t)kp * kstepb);
#pragma unroll
        for (int m = 0; m < 4; m++)
          b[m] = *(const dg_h8*)((const char*)col + (voff[m] + uo));
      };
      // k-step 2kp (a0: dims 8kp + g) then 2kp+1 (a1: dims 8kp + 4 + g)
      auto compute = [&](const dg_h8 (&b)[4], float a0, float a1) {
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
          for (int x = 0; x < 4; x++)
            acc[m][x] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a0, (float)b[m][x], acc[m][x], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
          for (int x = 0; x < 4; x++)
            acc[m][x] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a1, (float)b[m][4 + x], acc[m][x], 0, 0, 0);
      };
      auto qload = [&]() {
        dg_acc4 a = *ap;
        ap += QTM * 4;
        if (QTM < 16 && i >= QTM) a = dg_acc4{0.f, 0.f, 0.f, 0.f};
        return a;
      };

      // modulo schedule as in k_ivf_scan_mfma; a stage is one kp (8 dims),
      // a period four stages = 32 dims = two LDS reads
      issue(b0, 0);
      __builtin_amdgcn_sched_barrier(0);
      issue(b1, min(1, nkp - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b2, min(2, nkp - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b3, min(3, nkp - 1));
      __builtin_amdgcn_sched_barrier(0);
      int32_t kp = 0;
      for (; kp + 8 <= nkp; kp += 4) {  // the next period is whole too
        const dg_acc4 a = qload();
        const dg_acc4 c = qload();
        compute(b0, a.x, a.y);
        __builtin_amdgcn_sched_barrier(0);
        issue(b0, kp + 4);
        compute(b1, a.z, a.w);
        __builtin_amdgcn_sched_barrier(0);
        issue(b1, kp + 5);
        compute(b2, c.x, c.y);
        __builtin_amdgcn_sched_barrier(0);
        issue(b2, kp + 6);
        compute(b3, c.z, c.w);
        __builtin_amdgcn_sched_barrier(0);
        issue(b3, kp + 7);
      }
      if (kp + 4 < nkp) {  // whole period followed by a 1..3-stage one
        const int32_t rem = nkp - kp - 4;
        const dg_acc4 a = qload();
        const dg_acc4 c = qload();
        compute(b0, a.x, a.y);
        __builtin_amdgcn_sched_barrier(0);
        issue(b0, kp + 4);
        compute(b1, a.z, a.w);
        __builtin_amdgcn_sched_barrier(0);
        if (rem > 1) issue(b1, kp + 5);
        compute(b2, c.x, c.y);
        __builtin_amdgcn_sched_barrier(0);
        if (rem > 2) issue(b2, kp + 6);
        compute(b3, c.z, c.w);
        kp += 4;
      }
      {  // last period: 1..4 stages; absent stages are skipped
        const int32_t rem = nkp - kp;
        const dg_acc4 a = qload();
        const dg_acc4 c = qload();
        compute(b0, a.x, a.y);
        if (rem > 1) compute(b1, a.z, a.w);
        if (rem > 2) compute(b2, c.x, c.y);
        if (rem > 3) compute(b3, c.z, c.w);
      }
      if (FUSED)
        dg_scan_topk_epilogue_mfma(acc, cbase,
                                   (int64_t)(rb / (WAVE * 4)) * kf, vnorms,
                                   nrows, rb, row0, qt, metric, bitmap, kf,
                                   out);
      else
        dg_scan_store_epilogue_mfma(acc, cbase, vnorms, nrows, rb, row0, qt,
                                    metric, bitmap, out);
    }
  }
}

// ---------- SQ8 row storage (DG_STORAGE_SQ8) ----------
// Rows are stored as one byte per component (dg_sq8_core.h: the codec of
// faiss QT_8bit with per-dimension ranges); the query stays f32.  The scan
// does not decode a row: the affine map is folded into the query,
//   q . x = cq + sum_j (q_j * step_j) * code_j,
// so k_sq8_fold_query writes q' = q * step and cq once per batch, and
// k_ivf_scan_sq8 is k_ivf_scan_f16 with q' in its LDS image, the
// accumulators of a query preset to its cq and the bytes of a loaded dword
// converted (v_cvt_f32_ubyte0..3) straight into the B operand of the f32
// MFMA.  Keys, epilogues and everything after the scan see the full dot
// product.  dg_sq8_core.h documents the chunk layout: one 16-byte load per
// lane feeds four k-steps (16 dims) for four rows, and every load falls
// inside its chunk (lanes past nrows_pad re-read its first quad, absent
// prologue stages re-read its last kp), so the buffer needs no slack.
__global__ void k_sq8_encode_check(const float* __restrict__ in, int64_t n,
                                   int32_t d, const float* __restrict__ vmin,
                                   const float* __restrict__ vdiff,
                                   uint8_t* __restrict__ out,
                                   int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t j = (int32_t)(i % d);
  const float v = in[i];
  if (!(fabsf(v) <= 3.402823466e38f)) atomicOr(bad, 1);  // NaN and inf
  out[i] = dg_sq8_encode(v, vmin[j], vdiff[j]);
}

__global__ void k_row_norms_sq8(const uint8_t* __restrict__ x, int64_t n,
                                int32_t d, const float* __restrict__ vmin,
                                const float* __restrict__ vdiff,
                                float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) +
                      threadIdx.x / WAVE;
  if (row >= n) return;
  const int lane = threadIdx.x % WAVE;
  const uint8_t* p = x + (size_t)row * d;
  float s = 0.f;
  for (int32_t i = lane; i < d; i += WAVE) {
    const float v = dg_sq8_decode(p[i], vmin[i], vdiff[i]);
    s += v * v;
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (lane == 0) out[row] = s;
}

// out[i] = decoded row idx[i] of src, d bytes per row, d floats out
__global__ void k_gather_rows_by_index_sq8(const uint8_t* __restrict__ src,
                                           const int64_t* __restrict__ idx,
                                           int64_t n, int32_t d,
                                           const float* __restrict__ vmin,
                                           const float* __restrict__ vdiff,
                                           float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * d) return;
  const int64_t r = i / d;
  const int32_t c = (int32_t)(i - r * d);
  dst[i] = dg_sq8_decode(src[(size_t)idx[r] * d + c], vmin[c], vdiff[c]);
}

// one block per query: qp = q * step (f32), cq = sum q * (vmin + step / 2)
// accumulated in f64 and rounded once
__global__ void __launch_bounds__(256) k_sq8_fold_query(
    const float* __restrict__ q, int32_t d, const float* __restrict__ vmin,
    const float* __restrict__ step, float* __restrict__ qp,
    float* __restrict__ cq) {
  __shared__ double part[256 / WAVE];
  const float* src = q + (size_t)blockIdx.x * d;
  float* dst = qp + (size_t)blockIdx.x * d;
  double s = 0.0;
  for (int32_t j = threadIdx.x; j < d; j += blockDim.x) {
    const float v = src[j], st = step[j];
    dst[j] = v * st;
    s += (double)v * ((double)vmin[j] + 0.5 * (double)st);
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
  if (threadIdx.x % WAVE == 0) part[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 256 / WAVE; w++) t += part[w];
    cq[blockIdx.x] = (float)t;
  }
}

__global__ void __launch_bounds__(256) k_transpose_chunks_sq8(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const uint8_t* __restrict__ rowmajor, int32_t d, int32_t chunk_rows,
    uint8_t* __restrict__ tvec) {
  __shared__ uint8_t tile[64][68];
  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const int32_t d16 = dg_sq8_dims_pad(d);
  const uint8_t* src =
      rowmajor + (list_start + (int64_t)chunk * chunk_rows) * d;
  uint8_t* dst = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];

  const int tx = threadIdx.x % 64;
  const int ty = threadIdx.x / 64;
  for (int32_t r0 = 0; r0 < nrows_pad; r0 += 64) {
    for (int32_t i0 = 0; i0 < d16; i0 += 64) {
      __syncthreads();
      for (int rr = ty; rr < 64; rr += 4) {
        const int32_t r = r0 + rr;
        tile[rr][tx] = (r < nrows && i0 + tx < d)
                           ? src[(size_t)r * d + i0 + tx]
                           : (uint8_t)0;
      }
      __syncthreads();
      // 4 kp x 4 g x 16 quads = 256 16-byte groups per tile, one a thread
      const int quad = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3,
                kpl = threadIdx.x >> 6;
      const int32_t dim0 = i0 + 16 * kpl + g;  // h = 0
      const int32_t r = r0 + 4 * quad;
      if (dim0 < d16 && r < nrows_pad) {
        uint32_t w[4];  // one 16-byte store: chunks are 64-byte aligned
#pragma unroll
        for (int h = 0; h < 4; h++) {
          uint32_t v = 0;
#pragma unroll
          for (int x = 0; x < 4; x++)
            v |= (uint32_t)tile[4 * quad + x][16 * kpl + 4 * h + g] << (8 * x);
          w[h] = v;
        }
        *(uint4*)(dst + dg_sq8_chunk_offset(dim0, r, nrows_pad)) =
            make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
}

// FUSED: per-wave top-k into `out` (= partial, qp_off / q_cand_base unused);
// otherwise every candidate into `out` (= cand).  One dot-product body.
// qprime / cq are what k_sq8_fold_query wrote for this batch.
template <int QTM, bool FUSED>
__global__ void __launch_bounds__(256, 2) k_ivf_scan_sq8(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const uint8_t* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ qprime, const float* __restrict__ cq, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ out, int32_t kf, int32_t cpl_max) {
  static_assert(QTM <= 16 && QTM % 4 == 0, "one 16-query MFMA tile");
  // [nkp][QTM][4][4] floats (one 16-dim period per kp), cbase[QTM], cqs[QTM]
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __builtin_assume(d % 4 == 0 && d > 0);
  const int32_t nf4 = d >> 2;        // float4s of a query
  const int32_t nkp = (d + 15) >> 4;  // loads per lane and m: 16 dims each
  int64_t* cbase = (int64_t*)(smem + (size_t)nkp * QTM * 16);
  float* cqs = (float*)(cbase + QTM);

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const uint8_t* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  const int wave_id =
      __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  // bytes per kp (16 dims x nrows_pad bytes); a chunk is at most 8192 x 2048
  // bytes, so 32 bits hold every byte offset into it
  const uint32_t kstepb = (uint32_t)nrows_pad * 16u;

  // a list's query tiles are strided over grid.y, as in k_ivf_scan_f16
  for (int32_t t0 = QTM * (int32_t)blockIdx.y; t0 < nql;
       t0 += QTM * (int32_t)gridDim.y) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    // the LDS image of k_ivf_scan_mfma over q': float4 t of query j holds
    // dims 16kb + 4s + g (kb = t>>2, s = t&3); absent queries and dims are 0
    const int tid = wave_id * WAVE + dg_lane_id_fresh();
#pragma unroll 1
    for (int32_t j = 0; j < QTM; j++) {
      const float4* src =
          j < qt ? (const float4*)(qprime +
                                   (size_t)inv_q[iq0 + t0 + j] * d)
                 : nullptr;
      for (int32_t t = tid; t < nkp * 4; t += blockDim.x) {
        float4 v = float4{0.f, 0.f, 0.f, 0.f};
        if (src && t < nf4) v = src[t];
        float* dst = smem + ((size_t)(t >> 2) * QTM + j) * 16 + (t & 3);
        dst[0] = v.x;
        dst[4] = v.y;
        dst[8] = v.z;
        dst[12] = v.w;
      }
    }
    if (tid < QTM) {
      const int32_t j = tid;
      int64_t cb = 0;
      float c0 = 0.f;
      if (j < qt) {
        const int32_t q = inv_q[iq0 + t0 + j];
        const int32_t rank = inv_rank[iq0 + t0 + j];
        c0 = cq[q];
        if (FUSED)
          cb = ((((int64_t)q * nprobe + rank) * cpl_max + chunk) *
                (chunk_rows / (WAVE * 4))) * kf;
        else
          cb = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] +
               (int64_t)chunk * chunk_rows;
      }
      cbase[j] = cb;
      cqs[j] = c0;
    }
    __syncthreads();

    for (int32_t rb = wave_id * WAVE * 4; rb < nrows_pad; rb += 4 * WAVE * 4) {
      const int lane = dg_lane_id_fresh();
      const int g = lane >> 4, i = lane & 15;
      uint32_t voff[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int32_t rr = rb + 64 * m + 4 * i;
        voff[m] = ((uint32_t)g * (uint32_t)nrows_pad +
                   (uint32_t)(rr < nrows_pad ? rr : 0)) * 4u;
      }
      const dg_acc4* ap = (const dg_acc4*)smem + (i < QTM ? i : 0) * 4 + g;

      // the accumulators of query 4g + rq start at its cq (0 past QTM)
      dg_acc4 c4 = dg_acc4{0.f, 0.f, 0.f, 0.f};
      if (4 * g < QTM) c4 = *(const dg_acc4*)(cqs + 4 * g);
      dg_acc4 acc[4][4];
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int x = 0; x < 4; x++) acc[m][x] = c4;
      uint4 b0[4], b1[4], b2[4], b3[4];
      auto issue = [&](uint4 (&b)[4], int32_t kp) {
        const uint32_t uo =
            __builtin_amdgcn_readfirstlane((uint32_t)kp * kstepb);
#pragma unroll
        for (int m = 0; m < 4; m++)
          b[m] = *(const uint4*)(col + (voff[m] + uo));
      };
      // k-steps 4kp + h (a[h]: dims 16kp + 4h + g), h = 0..3 in order
      auto compute = [&](const uint4 (&b)[4], const dg_acc4 a) {
#pragma unroll
        for (int h = 0; h < 4; h++) {
#pragma unroll
          for (int m = 0; m < 4; m++) {
            const uint32_t w = h == 0   ? b[m].x
                               : h == 1 ? b[m].y
                               : h == 2 ? b[m].z
                                        : b[m].w;
#pragma unroll
            for (int x = 0; x < 4; x++)
              acc[m][x] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                  a[h], (float)((w >> (8 * x)) & 0xffu), acc[m][x], 0, 0, 0);
          }
        }
      };
      auto qload = [&]() {
        dg_acc4 a = *ap;
        ap += QTM * 4;
        if (QTM < 16 && i >= QTM) a = dg_acc4{0.f, 0.f, 0.f, 0.f};
        return a;
      };

      // modulo schedule as in k_ivf_scan_f16; a stage is one kp (16 dims
      // and one LDS read), a period four stages = 64 dims
      issue(b0, 0);
      __builtin_amdgcn_sched_barrier(0);
      issue(b1, min(1, nkp - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b2, min(2, nkp - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b3, min(3, nkp - 1));
      __builtin_amdgcn_sched_barrier(0);
      int32_t kp = 0;
      for (; kp + 8 <= nkp; kp += 4) {  // the next period is whole too
        compute(b0, qload());
        __builtin_amdgcn_sched_barrier(0);
        issue(b0, kp + 4);
        compute(b1, qload());
        __builtin_amdgcn_sched_barrier(0);
        issue(b1, kp + 5);
        compute(b2, qload());
        __builtin_amdgcn_sched_barrier(0);
        issue(b2, kp + 6);
        compute(b3, qload());
        __builtin_amdgcn_sched_barrier(0);
        issue(b3, kp + 7);
      }
      if (kp + 4 < nkp) {  // whole period followed by a 1..3-stage one
        const int32_t rem = nkp - kp - 4;
        compute(b0, qload());
        __builtin_amdgcn_sched_barrier(0);
        issue(b0, kp + 4);
        compute(b1, qload());
        __builtin_amdgcn_sched_barrier(0);
        if (rem > 1) issue(b1, kp + 5);
        compute(b2, qload());
        __builtin_amdgcn_sched_barrier(0);
        if (rem > 2) issue(b2, kp + 6);
        compute(b3, qload());
        kp += 4;
      }
      {  // last period: 1..4 stages; absent stages are skipped
        const int32_t rem = nkp - kp;
        compute(b0, qload());
        if (rem > 1) compute(b1, qload());
        if (rem > 2) compute(b2, qload());
        if (rem > 3) compute(b3, qload());
      }
      if (FUSED)
        dg_scan_topk_epilogue_mfma(acc, cbase,
                                   (int64_t)(rb / (WAVE * 4)) * kf, vnorms,
                                   nrows, rb, row0, qt, metric, bitmap, kf,
                                   out);
      else
        dg_scan_store_epilogue_mfma(acc, cbase, vnorms, nrows, rb, row0, qt,
                                    metric, bitmap, out);
    }
  }
}

// ---------- pair scan: two query tiles per pass over a chunk's rows ------
// A list probed by more than 16 queries costs k_ivf_scan_mfma one HBM pass
// over its chunk per 16-query tile.  k_ivf_scan_mfma2 feeds each k-step's
// four row loads to 32 MFMAs, into one accumulator set per tile of a pair
// (tiles 2p and 2p+1 of the list's probing queries), and runs the epilogue
// once per set; dg_scan_split.h says which tiles it takes and which stay
// with k_ivf_scan_mfma.  Every (query, row) dot is the same k-ordered chain
// and every slot gets the same bits as from k_ivf_scan_mfma.
//
// A 32-query LDS image would leave one block per CU, so the A operand comes
// from global memory: k_query_image writes every query once in the operand
// order of the LDS image, [q][d/16 period][g 4][s 4] for dim 16kb+4s+g
// (absent dims zero), plus one all-zero query at index nq for the absent
// queries of a partial second tile.  Lane (g,i) loads its float4 of tile t
// from image[inv_q[..16t+i]] one period ahead, in the row loads' pipeline.
__global__ void k_query_image(const float* __restrict__ queries, int64_t nq,
                              int32_t d, float* __restrict__ image) {
  const int32_t nks = d >> 2;
  const int32_t nf4 = ((nks + 3) >> 2) * 4;  // float4s per query image
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (nq + 1) * nf4) return;
  const int64_t q = idx / nf4;
  const int32_t t = (int32_t)(idx - q * nf4);
  float4 v = float4{0.f, 0.f, 0.f, 0.f};
  if (q < nq && t < nks) v = ((const float4*)(queries + (size_t)q * d))[t];
  float* dst = image + ((size_t)q * nf4 + (t & ~3)) * 4 + (t & 3);
  dst[0] = v.x;
  dst[4] = v.y;
  dst[8] = v.z;
  dst[12] = v.w;
}

// SHORT is d <= 16, a single period: the instance for longer rows knows
// that its dim loop runs at least once, so the accumulators have one
// definition at the loop head instead of a merge with the zero-trip path
// (which the register allocator resolves through scratch).
template <bool SHORT>
__global__ void __launch_bounds__(256, 2) k_ivf_scan_mfma2(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ image, int32_t zero_q, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ partial, int32_t kf, int32_t cpl_max) {
  constexpr int QT = kScanTileQ;
  __shared__ int64_t cbase[2 * QT];
  __builtin_assume(d % 4 == 0 && d > 0);
  const int32_t nks = d >> 2;           // k-steps of 4 dims
  const int32_t nper = (nks + 3) >> 2;  // periods of 4 k-steps

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;
  // blockIdx.y strides over the list's pairs; most units have none
  const int32_t npairs = dg_scan_pairs(nql, true);
  if ((int32_t)blockIdx.y >= npairs) return;
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;

  const int wave_id =
      __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const uint32_t kstepb = (uint32_t)nrows_pad * 16u;
  // bytes per query image; the host launches this kernel only when the
  // whole image (nq + 1 queries) is below 4 GiB
  const uint32_t qimgb = (uint32_t)nper * 64u;

  for (int32_t p = (int32_t)blockIdx.y; p < npairs; p += (int32_t)gridDim.y) {
    const int32_t t0 = 2 * QT * p;
    // tile 2p is whole; tile 2p+1 holds 1..16 queries
    const int32_t qt1 = min(QT, nql - t0 - QT);
    __syncthreads();
    {
      const int tid = wave_id * WAVE + dg_lane_id_fresh();
      if (tid < 2 * QT) {
        int64_t cb = 0;
        if (tid < QT + qt1)
          cb = ((((int64_t)inv_q[iq0 + t0 + tid] * nprobe +
                  inv_rank[iq0 + t0 + tid]) * cpl_max + chunk) *
                (chunk_rows / (WAVE * 4))) * kf;
        cbase[tid] = cb;
      }
    }
    __syncthreads();

    for (int32_t rb = wave_id * WAVE * 4; rb < nrows_pad; rb += 4 * WAVE * 4) {
      const int64_t wslot = (int64_t)(rb / (WAVE * 4)) * kf;
      const int lane = dg_lane_id_fresh();
      const int g = lane >> 4, i = lane & 15;
      uint32_t voff[4];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const int32_t rr = rb + 64 * m + 4 * i;
        voff[m] = ((uint32_t)g * (uint32_t)nrows_pad +
                   (uint32_t)(rr < nrows_pad ? rr : 0)) * 4u;
      }
      // byte offsets of the lane's operand rows in the two queries' images;
      // absent queries of the second tile read the zero query
      const uint32_t aoff0 =
          (uint32_t)inv_q[iq0 + t0 + i] * qimgb + (uint32_t)g * 16u;
      const uint32_t aoff1 =
          (uint32_t)(i < qt1 ? inv_q[iq0 + t0 + QT + i] : zero_q) * qimgb +
          (uint32_t)g * 16u;

      float z = 0.f;
      asm volatile("" : "+v"(z));
      dg_acc4 acc0[4][4], acc1[4][4];
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int x = 0; x < 4; x++) {
          acc0[m][x] = dg_acc4{z, z, z, z};
          acc1[m][x] = dg_acc4{z, z, z, z};
        }
      dg_acc4 b0[4], b1[4], b2[4], b3[4];
      dg_acc4 a0, a1, n0, n1;  // this period's operands, the next period's
      auto issue = [&](dg_acc4 (&b)[4], int32_t ks) {
        const uint32_t uo =
            __builtin_amdgcn_readfirstlane((uint32_t)ks * kstepb);
#pragma unroll
        for (int m = 0; m < 4; m++)
          b[m] = *(const dg_acc4*)((const char*)col + (voff[m] + uo));
      };
      auto aissue = [&](dg_acc4& x0, dg_acc4& x1, int32_t per) {
        const uint32_t po =
            __builtin_amdgcn_readfirstlane((uint32_t)per * 64u);
        x0 = *(const dg_acc4*)((const char*)image + (aoff0 + po));
        x1 = *(const dg_acc4*)((const char*)image + (aoff1 + po));
      };
      auto compute = [&](const dg_acc4 (&b)[4], float x0, float x1) {
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
          for (int x = 0; x < 4; x++) {
            acc0[m][x] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                x0, b[m][x], acc0[m][x], 0, 0, 0);
            acc1[m][x] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                x1, b[m][x], acc1[m][x], 0, 0, 0);
          }
      };

      // the modulo schedule of k_ivf_scan_mfma; the next period's operands
      // are issued just ahead of stage 0's re-issue, so the wait for that
      // stage at the next period's head covers them
      aissue(a0, a1, 0);
      issue(b0, 0);
      __builtin_amdgcn_sched_barrier(0);
      issue(b1, min(1, nks - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b2, min(2, nks - 1));
      __builtin_amdgcn_sched_barrier(0);
      issue(b3, min(3, nks - 1));
      __builtin_amdgcn_sched_barrier(0);
      int32_t ks = 0;
      if (!SHORT) __builtin_assume(nks > 4);
      // (one loop form for every period that has a successor: where the
      // successor has 1..3 k-steps its absent stages re-read the last
      // column, as in the prologue, and are never consumed)
      for (; !SHORT && ks + 4 < nks; ks += 4) {
        compute(b0, a0.x, a1.x);
        __builtin_amdgcn_sched_barrier(0);
        aissue(n0, n1, (ks >> 2) + 1);
        issue(b0, ks + 4);
        compute(b1, a0.y, a1.y);
        __builtin_amdgcn_sched_barrier(0);
        issue(b1, min(ks + 5, nks - 1));
        compute(b2, a0.z, a1.z);
        __builtin_amdgcn_sched_barrier(0);
        issue(b2, min(ks + 6, nks - 1));
        compute(b3, a0.w, a1.w);
        __builtin_amdgcn_sched_barrier(0);
        issue(b3, min(ks + 7, nks - 1));
        a0 = n0;
        a1 = n1;
      }
      {  // last period: 1..4 k-steps; absent steps are skipped, not padded
        const int32_t rem = nks - ks;
        compute(b0, a0.x, a1.x);
        if (rem > 1) compute(b1, a0.y, a1.y);
        if (rem > 2) compute(b2, a0.z, a1.z);
        if (rem > 3) compute(b3, a0.w, a1.w);
      }
      dg_scan_topk_epilogue_mfma(acc0, cbase, wslot, vnorms, nrows, rb, row0,
                                 QT, metric, bitmap, kf, partial);
      dg_scan_topk_epilogue_mfma(acc1, cbase + QT, wslot, vnorms, nrows, rb,
                                 row0, qt1, metric, bitmap, kf, partial);
    }
  }
}

// ---------- generalized drain pipeline (v5, DG_SCAN_VARIANT=16..18) ----
// SAFE-mode generalization of k_ivf_scan_pipe: S stages x 4 dims issued as
// one batch at block end, ONE vmcnt(0) drain at the next block's head
// (tied per stage before its compute), amortizing the exposed HBM latency
// over 4*S dims instead of 4.  All waits are full drains, so the LLVM
// in-flight-register hazards of the counted variants cannot occur.
template <int QTM, int S>
__global__ void __launch_bounds__(256, 1) k_ivf_scan_pipe3(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  constexpr int RPL = 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [QTM * d]
  int64_t* cbase = (int64_t*)(smem + (size_t)QTM * d);          // [QTM]

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  __builtin_assume(d % 4 == 0 && d > 0);

  for (int32_t t0 = 0; t0 < nql; t0 += QTM) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    for (int32_t j = 0; j < qt; j++) {
      int32_t q = inv_q[iq0 + t0 + j];
      const float4* src = (const float4*)(queries + (size_t)q * d);
      float4* dst = (float4*)(smem + (size_t)j * d);
      for (int i = threadIdx.x; i < d / 4; i += blockDim.x) dst[i] = src[i];
    }
    for (size_t i = (size_t)qt * d + threadIdx.x; i < (size_t)QTM * d;
         i += blockDim.x)
      smem[i] = 0.f;
    if (threadIdx.x < QTM) {
      int32_t j = threadIdx.x;
      if (j < qt) {
        int32_t q = inv_q[iq0 + t0 + j];
        int32_t rank = inv_rank[iq0 + t0 + j];
        cbase[j] = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] -
                   list_start;
      } else {
        cbase[j] = 0;
      }
    }
    __syncthreads();

    for (int32_t rb = wave_id * WAVE * RPL; rb < nrows_pad;
         rb += 4 * WAVE * RPL) {
      const int32_t rr0 = rb + lane * RPL;
      if (rr0 >= nrows_pad) continue;
      float acc[QTM][RPL];
#pragma unroll
      for (int j = 0; j < QTM; j++)
#pragma unroll
        for (int x = 0; x < RPL; x++) acc[j][x] = 0.f;

      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // prior emit stores
      const char* colp0 = (const char*)(col + rr0);
      const size_t cstride = (size_t)nrows_pad * 4;
      dg_f4 buf[S][4];
      auto issue_block = [&](int32_t ib) {
#pragma unroll
        for (int i = 0; i < S; i++)
#pragma unroll
          for (int u = 0; u < 4; u++)
            DG_GLOAD4(buf[i][u],
                      colp0 + (size_t)(ib + 4 * i + u) * cstride);
      };
      auto compute4 = [&](const dg_f4 (&b)[4], int32_t ib) {
#pragma unroll
        for (int j = 0; j < QTM; j++) {
          const float* qp = smem + (size_t)j * d + ib;
          const float2 qa = *(const float2*)qp;
          const float2 qb = *(const float2*)(qp + 2);
          const float qv[4] = {qa.x, qa.y, qb.x, qb.y};
#pragma unroll
          for (int u = 0; u < 4; u++)
#pragma unroll
            for (int x = 0; x < RPL; x++) acc[j][x] += b[u][x] * qv[u];
        }
      };
      constexpr int BD = 4 * S;  // dims per block
      int32_t base = 0;
      if (d >= BD) {
        issue_block(0);
        for (; base + BD <= d; base += BD) {
          const bool more = base + 2 * BD <= d;
#pragma unroll
          for (int i = 0; i < S; i++) {
            DG_WAITV(0, buf[i]);  // first drains everything; rest order
            compute4(buf[i], base + 4 * i);
          }
          if (more) issue_block(base + BD);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      // tail < BD dims: compiler-managed loads
      const float* colf = col + rr0;
      for (int32_t ib = base; ib < d; ib += 4) {
        float4 c[4];
#pragma unroll
        for (int u = 0; u < 4; u++)
          c[u] = (ib + u < d)
                     ? *(const float4*)(colf + (size_t)(ib + u) * nrows_pad)
                     : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < QTM; j++) {
          const float* qp = smem + (size_t)j * d + ib;
#pragma unroll
          for (int u = 0; u < 4 && ib + u < d; u++) {
            const float qv = qp[u];
            acc[j][0] += c[u].x * qv;
            acc[j][1] += c[u].y * qv;
            acc[j][2] += c[u].z * qv;
            acc[j][3] += c[u].w * qv;
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#pragma unroll
      for (int j = 0; j < QTM; j++) {
        if (j < qt) {
          const int64_t cb = cbase[j] + row0 + rr0;
#pragma unroll
          for (int x = 0; x < RPL; x++) {
            const int32_t rl = rr0 + x;
            if (rl < nrows) {
              const int64_t r = row0 + rl;
              bool pass = true;
              if (bitmap) pass = (bitmap[r >> 5] >> (r & 31)) & 1;
              float key = (metric == 0) ? vnorms[r] - 2.0f * acc[j][x]
                                        : -acc[j][x];
              cand[cb + x] = pass ? pack_cand(key, (uint32_t)r) : kCandEmpty;
            }
          }
        }
      }
    }
  }
}


template <int QTM>
__global__ void __launch_bounds__(256, 1) k_ivf_scan_pipe4(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  constexpr int RPL = 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int64_t* cbase = (int64_t*)(smem + (size_t)QTM * d);
  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;
  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  __builtin_assume(d % 4 == 0 && d > 0);
  for (int32_t t0 = 0; t0 < nql; t0 += QTM) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    for (int32_t j = 0; j < qt; j++) {
      int32_t q = inv_q[iq0 + t0 + j];
      const float4* src = (const float4*)(queries + (size_t)q * d);
      float4* dst = (float4*)(smem + (size_t)j * d);
      for (int i = threadIdx.x; i < d / 4; i += blockDim.x) dst[i] = src[i];
    }
    for (size_t i = (size_t)qt * d + threadIdx.x; i < (size_t)QTM * d;
         i += blockDim.x)
      smem[i] = 0.f;
    if (threadIdx.x < QTM) {
      int32_t j = threadIdx.x;
      if (j < qt) {
        int32_t q = inv_q[iq0 + t0 + j];
        int32_t rank = inv_rank[iq0 + t0 + j];
        cbase[j] = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] -
                   list_start;
      } else {
        cbase[j] = 0;
      }
    }
    __syncthreads();
    for (int32_t rb = wave_id * WAVE * RPL; rb < nrows_pad;
         rb += 4 * WAVE * RPL) {
      const int32_t rr0 = rb + lane * RPL;
      if (rr0 >= nrows_pad) continue;
      if (QTM >= 16 && qt <= QTM / 2)
        dg_scan_rows_body2<(QTM >= 16 ? QTM / 2 : QTM)>(
            smem, cbase, col, vnorms, d, nrows, nrows_pad, rr0, row0, qt,
            metric, bitmap, cand);
      else
        dg_scan_rows_body2<QTM>(smem, cbase, col, vnorms, d, nrows,
                                nrows_pad, rr0, row0, qt, metric, bitmap,
                                cand);
    }
  }
}

// ---------- fused-stage asm scan (v4, DG_SCAN_VARIANT=13) ----------
// The v3 kernel's separate issue/wait asms are not airtight: LLVM may copy
// or reuse an in-flight load's destination registers between the asm
// statements (it models asm loads as completing instantly; verified in the
// emitted code by a static hazard scan).  Here each 8-dim stage is ONE asm
// block — 8 global_load_dwordx4 into the next bank, address bumps, and the
// counted s_waitcnt vmcnt(8) that retires the CURRENT bank — so no
// compiler-scheduled instruction can fall between a load and the wait that
// guards its window.  Two banks ping-pong; the current bank's values are
// tied through ("+v") so their consumers order after the wait.
#define DG_STAGE8(c0, c1, c2, c3, c4, c5, c6, c7, n0, n1, n2, n3, n4, n5,  \
                  n6, n7, addr, stride)                                    \
  asm volatile("global_load_dwordx4 %9, %8, off\n\t"                       \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "global_load_dwordx4 %10, %8, off\n\t"                      \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "global_load_dwordx4 %11, %8, off\n\t"                      \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "global_load_dwordx4 %12, %8, off\n\t"                      \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "global_load_dwordx4 %13, %8, off\n\t"                      \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "global_load_dwordx4 %14, %8, off\n\t"                      \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "global_load_dwordx4 %15, %8, off\n\t"                      \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "global_load_dwordx4 %16, %8, off\n\t"                      \
               "v_lshl_add_u64 %8, %8, 0, %17\n\t"                         \
               "s_waitcnt vmcnt(8)"                                        \
               : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3), "+v"(c4),         \
                 "+v"(c5), "+v"(c6), "+v"(c7), "+v"(addr), "=&v"(n0),      \
                 "=&v"(n1), "=&v"(n2), "=&v"(n3), "=&v"(n4), "=&v"(n5),    \
                 "=&v"(n6), "=&v"(n7)                                      \
               : "v"(stride))

// prologue: issue one bank, no wait
#define DG_ISSUE8(n0, n1, n2, n3, n4, n5, n6, n7, addr, stride)            \
  asm volatile("global_load_dwordx4 %1, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9\n\t"                          \
               "global_load_dwordx4 %2, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9\n\t"                          \
               "global_load_dwordx4 %3, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9\n\t"                          \
               "global_load_dwordx4 %4, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9\n\t"                          \
               "global_load_dwordx4 %5, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9\n\t"                          \
               "global_load_dwordx4 %6, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9\n\t"                          \
               "global_load_dwordx4 %7, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9\n\t"                          \
               "global_load_dwordx4 %8, %0, off\n\t"                       \
               "v_lshl_add_u64 %0, %0, 0, %9"                              \
               : "+v"(addr), "=&v"(n0), "=&v"(n1), "=&v"(n2), "=&v"(n3),   \
                 "=&v"(n4), "=&v"(n5), "=&v"(n6), "=&v"(n7)                \
               : "v"(stride))

// wait draining everything, tying one bank's consumers behind it
#define DG_DRAIN8(b0, b1, b2, b3, b4, b5, b6, b7)                          \
  asm volatile("s_waitcnt vmcnt(0)"                                        \
               : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4),         \
                 "+v"(b5), "+v"(b6), "+v"(b7))

template <int QTM>
__global__ void __launch_bounds__(256, 1) k_ivf_scan_pipe2(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  constexpr int RPL = 4;
  extern __shared__ __attribute__((aligned(16))) float smem[];  // [QTM * d]
  int64_t* cbase = (int64_t*)(smem + (size_t)QTM * d);          // [QTM]

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  __builtin_assume(d % 4 == 0 && d > 0);

  for (int32_t t0 = 0; t0 < nql; t0 += QTM) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    for (int32_t j = 0; j < qt; j++) {
      int32_t q = inv_q[iq0 + t0 + j];
      const float4* src = (const float4*)(queries + (size_t)q * d);
      float4* dst = (float4*)(smem + (size_t)j * d);
      for (int i = threadIdx.x; i < d / 4; i += blockDim.x) dst[i] = src[i];
    }
    for (size_t i = (size_t)qt * d + threadIdx.x; i < (size_t)QTM * d;
         i += blockDim.x)
      smem[i] = 0.f;
    if (threadIdx.x < QTM) {
      int32_t j = threadIdx.x;
      if (j < qt) {
        int32_t q = inv_q[iq0 + t0 + j];
        int32_t rank = inv_rank[iq0 + t0 + j];
        cbase[j] = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] -
                   list_start;
      } else {
        cbase[j] = 0;
      }
    }
    __syncthreads();

    for (int32_t rb = wave_id * WAVE * RPL; rb < nrows_pad;
         rb += 4 * WAVE * RPL) {
      const int32_t rr0 = rb + lane * RPL;
      if (rr0 >= nrows_pad) continue;
      float acc[QTM][RPL];
#pragma unroll
      for (int j = 0; j < QTM; j++)
#pragma unroll
        for (int x = 0; x < RPL; x++) acc[j][x] = 0.f;

      // drain previous-tile vmem so the fused counts are exact
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

      const size_t cstride = (size_t)nrows_pad * 4;
      uint64_t addr = (uint64_t)(uintptr_t)(col + rr0);
      const uint64_t stride = cstride;
      dg_f4 a0, a1, a2, a3, a4, a5, a6, a7;
      dg_f4 b0, b1, b2, b3, b4, b5, b6, b7;

      // 8 dims of one bank against all staged queries.  The sched barrier
      // every 4 queries stops the scheduler from hoisting ALL queries' LDS
      // reads at once (measured: 96 live query registers, pushing the
      // allocator into AGPR stashes of the in-flight bank = reads of
      // pending load destinations).
      auto compute8 = [&](const dg_f4& x0, const dg_f4& x1, const dg_f4& x2,
                          const dg_f4& x3, const dg_f4& x4, const dg_f4& x5,
                          const dg_f4& x6, const dg_f4& x7, int32_t ib) {
        const dg_f4* xs[8] = {&x0, &x1, &x2, &x3, &x4, &x5, &x6, &x7};
#pragma unroll
        for (int j = 0; j < QTM; j++) {
          const float* qp = smem + (size_t)j * d + ib;
#pragma unroll
          for (int h = 0; h < 4; h++) {
            const float2 qq = *(const float2*)(qp + 2 * h);
            const dg_f4& ca = *xs[2 * h];
            const dg_f4& cb = *xs[2 * h + 1];
#pragma unroll
            for (int x = 0; x < RPL; x++)
              acc[j][x] += ca[x] * qq.x + cb[x] * qq.y;
          }
          if ((j & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
      };

      int32_t base = 0;
      if (d >= 16) {
        DG_ISSUE8(a0, a1, a2, a3, a4, a5, a6, a7, addr, stride);
        for (; base + 16 <= d; base += 16) {
          // sched barriers pin each compute phase between its stage asms:
          // without them the scheduler sinks FMA chunks past the next
          // stage, doubling bank liveness and pushing the allocator into
          // AGPR stashes of in-flight destinations
          DG_STAGE8(a0, a1, a2, a3, a4, a5, a6, a7, b0, b1, b2, b3, b4, b5,
                    b6, b7, addr, stride);
          __builtin_amdgcn_sched_barrier(0);
          compute8(a0, a1, a2, a3, a4, a5, a6, a7, base);
          __builtin_amdgcn_sched_barrier(0);
          DG_STAGE8(b0, b1, b2, b3, b4, b5, b6, b7, a0, a1, a2, a3, a4, a5,
                    a6, a7, addr, stride);
          __builtin_amdgcn_sched_barrier(0);
          compute8(b0, b1, b2, b3, b4, b5, b6, b7, base + 8);
          __builtin_amdgcn_sched_barrier(0);
        }
        DG_DRAIN8(a0, a1, a2, a3, a4, a5, a6, a7);
      }
      // tail (< 16 dims): compiler-managed loads
      const float* colp = col + rr0;
      for (int32_t ib = base; ib < d; ib += 4) {
        float4 c[4];
#pragma unroll
        for (int u = 0; u < 4; u++)
          c[u] = (ib + u < d) ? *(const float4*)(colp +
                                                 (size_t)(ib + u) * nrows_pad)
                              : float4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < QTM; j++) {
          const float* qp = smem + (size_t)j * d + ib;
#pragma unroll
          for (int u = 0; u < 4 && ib + u < d; u++) {
            const float qv = qp[u];
            acc[j][0] += c[u].x * qv;
            acc[j][1] += c[u].y * qv;
            acc[j][2] += c[u].z * qv;
            acc[j][3] += c[u].w * qv;
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#pragma unroll
      for (int j = 0; j < QTM; j++) {
        if (j < qt) {
          const int64_t cb = cbase[j] + row0 + rr0;
#pragma unroll
          for (int x = 0; x < RPL; x++) {
            const int32_t rl = rr0 + x;
            if (rl < nrows) {
              const int64_t r = row0 + rl;
              bool pass = true;
              if (bitmap) pass = (bitmap[r >> 5] >> (r & 31)) & 1;
              float key = (metric == 0) ? vnorms[r] - 2.0f * acc[j][x]
                                        : -acc[j][x];
              cand[cb + x] = pass ? pack_cand(key, (uint32_t)r) : kCandEmpty;
            }
          }
        }
      }
    }
  }
}

// ---------- glds scan (v3 experiment, DG_SCAN_VARIANT=7) ----------
// Column data streams HBM -> LDS via global_load_lds into a per-wave
// private ring (each wave owns a 256-row quarter of the chunk, so no
// cross-wave hand-off and no barriers in the steady loop; counted vmcnt
// waits only).  Consumers read columns from LDS (conflict-free b128) and
// accumulate lane-private dots as in v2.  1 block/CU (LDS-bound).
template <int QTM, int DEPTH>
__global__ void __launch_bounds__(256, 1) k_ivf_scan_glds(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  // LDS: [QTM*d] query tile | per-wave rings [4][DEPTH][4*256] | cbase[QTM]
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int SLOT = 4 * 256;  // 4 dims x 256 rows (f32)
  float* ring_all = smem + (size_t)QTM * d;
  int64_t* cbase = (int64_t*)(ring_all + 4 * DEPTH * SLOT);

  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const float* col = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];
  const int64_t row0 = list_start + (int64_t)chunk * chunk_rows;
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;

  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  __builtin_assume(d % 4 == 0 && d > 0);
  float* ring = ring_all + wave_id * DEPTH * SLOT;
  const int32_t wrow0 = wave_id * 256;          // this wave's row quarter
  if (wrow0 >= nrows_pad) {
    // idle quarter still participates in the staging barriers below
  }
  const int32_t rr0 = wrow0 + lane * 4;         // this lane's 4 rows
  const int nslots = d / 4;                     // slots per full pass

  for (int32_t t0 = 0; t0 < nql; t0 += QTM) {
    const int32_t qt = min(QTM, nql - t0);
    __syncthreads();
    for (int32_t j = 0; j < qt; j++) {
      int32_t q = inv_q[iq0 + t0 + j];
      const float4* src = (const float4*)(queries + (size_t)q * d);
      float4* dst = (float4*)(smem + (size_t)j * d);
      for (int i = threadIdx.x; i < d / 4; i += blockDim.x) dst[i] = src[i];
    }
    for (size_t i = (size_t)qt * d + threadIdx.x; i < (size_t)QTM * d;
         i += blockDim.x)
      smem[i] = 0.f;
    if (threadIdx.x < QTM) {
      int32_t j = threadIdx.x;
      if (j < qt) {
        int32_t q = inv_q[iq0 + t0 + j];
        int32_t rank = inv_rank[iq0 + t0 + j];
        cbase[j] = q_cand_base[q] + qp_off[(int64_t)q * nprobe + rank] -
                   list_start;
      } else {
        cbase[j] = 0;
      }
    }
    __syncthreads();
    if (wrow0 < nrows_pad) {
      float acc[QTM][4];
#pragma unroll
      for (int j = 0; j < QTM; j++)
#pragma unroll
        for (int x = 0; x < 4; x++) acc[j][x] = 0.f;

      // issue one slot: 4 glds of 1 KiB (dim column slice for this quarter)
      auto issue = [&](int32_t slot_i /* dim block index */) {
        float* ldst = ring + (slot_i % DEPTH) * SLOT;
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const float* gsrc =
              col + (size_t)(slot_i * 4 + u) * nrows_pad + wrow0 + lane * 4;
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) uint32_t*)gsrc,
              (__attribute__((address_space(3))) uint32_t*)(ldst + u * 256),
              16, 0, 0);
        }
      };
      auto consume = [&](int32_t slot_i) {
        const float* sl = ring + (slot_i % DEPTH) * SLOT + lane * 4;
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const float4 c4 = *(const float4*)(sl + u * 256);
#pragma unroll
          for (int j = 0; j < QTM; j++) {
            const float qv = smem[(size_t)j * d + slot_i * 4 + u];
            acc[j][0] += c4.x * qv;
            acc[j][1] += c4.y * qv;
            acc[j][2] += c4.z * qv;
            acc[j][3] += c4.w * qv;
          }
        }
      };
      const int pre = min(DEPTH, nslots);
      for (int s = 0; s < pre; s++) issue(s);
      for (int s = 0; s < nslots; s++) {
        // wait until slot s's 4 glds landed; leave the younger slots'
        // glds in flight: outstanding after wait = 4*(issued - s - 1).
        // asm form with memory clobber so ds_reads can't hoist above it
        // (counted waits only — a vmcnt(0) here would drain the ring).
        const int n_out = 4 * (min(nslots, s + DEPTH) - s - 1);
        switch (n_out) {
          case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
          case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
          case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
          case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
          case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
          case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
          default: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
        }
        consume(s);
        if (s + DEPTH < nslots) issue(s + DEPTH);
      }
      (void)pre;
      // emit (guards, not breaks — see v2)
#pragma unroll
      for (int j = 0; j < QTM; j++) {
        if (j < qt) {
          const int64_t cb = cbase[j] + row0 + rr0;
#pragma unroll
          for (int x = 0; x < 4; x++) {
            const int32_t rl = rr0 + x;
            if (rl < nrows) {
              const int64_t r = row0 + rl;
              bool pass = true;
              if (bitmap) pass = (bitmap[r >> 5] >> (r & 31)) & 1;
              float key = (metric == 0) ? vnorms[r] - 2.0f * acc[j][x]
                                        : -acc[j][x];
              cand[cb + x] = pass ? pack_cand(key, (uint32_t)r)
                                  : kCandEmpty;
            }
          }
        }
      }
    }
  }
}

// wrappers: same body, different register budgets.  The (256,1) form lets
// the allocator use 209 VGPRs (2 blocks/CU, LDS would allow 3); the
// (256,3) form caps at 168 VGPRs for 3 waves/SIMD at the cost of possible
// cold spills -- A/B'd via DG_SCAN_VARIANT.
template <int QTM, int RPL>
__global__ void __launch_bounds__(256, 1) k_ivf_scan_col(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  ivf_scan_col_body<QTM, RPL>(units, csr_offsets, chunk_off, chunk_base,
                              tvec, vnorms, queries, d, inv_offsets, inv_q,
                              inv_rank, qp_off, q_cand_base, nprobe, metric,
                              bitmap, chunk_rows, cand);
}

template <int QTM, int RPL>
__global__ void __launch_bounds__(256, 1) k_ivf_scan_col_nt(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  ivf_scan_col_body<QTM, RPL, true>(units, csr_offsets, chunk_off, chunk_base,
                                    tvec, vnorms, queries, d, inv_offsets,
                                    inv_q, inv_rank, qp_off, q_cand_base,
                                    nprobe, metric, bitmap, chunk_rows, cand);
}

template <int QTM, int RPL>
__global__ void __launch_bounds__(256, 3) k_ivf_scan_col_hi(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const float* __restrict__ tvec, const float* __restrict__ vnorms,
    const float* __restrict__ queries, int32_t d,
    const int32_t* __restrict__ inv_offsets, const int32_t* __restrict__ inv_q,
    const int32_t* __restrict__ inv_rank, const int64_t* __restrict__ qp_off,
    const int64_t* __restrict__ q_cand_base, int32_t nprobe, int metric,
    const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  ivf_scan_col_body<QTM, RPL>(units, csr_offsets, chunk_off, chunk_base,
                              tvec, vnorms, queries, d, inv_offsets, inv_q,
                              inv_rank, qp_off, q_cand_base, nprobe, metric,
                              bitmap, chunk_rows, cand);
}

// tiled row-major -> column-major chunk transpose (finalize step).
// One block per (list, chunk) unit over ALL chunks; LDS 64x65 tile.
// T = float for the IVF-Flat columns, uint32_t for the packed words of the
// binary indexes (d = words per row there).
template <typename T>
__global__ void k_transpose_chunks(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const T* __restrict__ rowmajor, int32_t d, int32_t chunk_rows,
    T* __restrict__ tvec) {
  __shared__ T tile[64][65];
  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t nrows_pad = (nrows + 3) & ~3;
  const T* src = rowmajor + (list_start + (int64_t)chunk * chunk_rows) * d;
  T* dst = tvec + chunk_base[chunk_off[list] + (int32_t)chunk];

  const int tx = threadIdx.x % 64;  // dim within tile on read, row on write
  const int ty = threadIdx.x / 64;  // 4 groups
  for (int32_t r0 = 0; r0 < nrows; r0 += 64) {
    for (int32_t i0 = 0; i0 < d; i0 += 64) {
      __syncthreads();
      for (int rr = ty; rr < 64; rr += 4) {
        int32_t r = r0 + rr;
        tile[rr][tx] = (r < nrows && i0 + tx < d)
                           ? src[(size_t)r * d + i0 + tx]
                           : T(0);
      }
      __syncthreads();
      for (int ii = ty; ii < 64; ii += 4) {
        int32_t i = i0 + ii;
        int32_t r = r0 + tx;
        if (i < d && r < nrows_pad)
          dst[(size_t)i * nrows_pad + r] = tile[tx][ii];
      }
    }
  }
}

// ---------- hand MFMA f32 dots GEMM ----------
// C[M][N] = X[M][d] . Y[N][d]^T, all row-major — the coarse
// query x centroid assignment GEMM the north star names as THE MFMA target
// (SURVEY.md §8a row a4), also used for the Flat exact-scan dots.
// gfx950 f32-input MFMA v_mfma_f32_32x32x2_f32: exact f32 (a k-ordered fmaf
// chain, cdna_hip_programming.md §3), 64 cyc issue = dependent latency, so
// one accumulator per wave reaches the 157 TF f32 rate.  Block = 4 waves =
// 64x64 tile (each wave one 32x32 accumulator, 16 AGPRs), BK=16 double-
// buffered LDS (2 x 2 x 64x16 f32 = 16 KB), A/B operands read from LDS as
// b64 (two k-steps per read).
__global__ void __launch_bounds__(256, 2) k_dots_mfma(
    const float* __restrict__ X, const float* __restrict__ Y, int64_t M,
    int64_t N, int32_t K, float* __restrict__ C, int64_t ldc) {
  // 128x128 block, 4 waves as 2x2 of 64x64, each wave 2x2 accumulators of
  // 32x32 => 64 MFMA per wave between barriers (the guide's untuned
  // 128x128x32 f32 shape reaches 122 TF; a 64x64/BK16 first cut measured
  // 27 TF — barrier overhead per 8 MFMAs dominated).
  constexpr int BM = 128, BN = 128, BK = 32;
  // BK+4 stride: rows are 144 B = 16 B-aligned, so staging writes are
  // ds_write_b128 (the round-1 BK+1 odd stride forced 32 SCALAR b32
  // writes per thread per stage — the staging cost, not the MFMAs, capped
  // that kernel at 57 TF).  Column reads pay a 2-way bank conflict
  // (rows r and r+16 share banks at stride 36) — measured cheaper than
  // the scalar-write staging.
  __shared__ float lx[2][BM][BK + 4];
  __shared__ float ly[2][BN][BK + 4];
  using f32x16 = __attribute__((__vector_size__(16 * sizeof(float)))) float;

  const int64_t m0 = (int64_t)blockIdx.y * BM;
  const int64_t n0 = (int64_t)blockIdx.x * BN;
  const int wave_id = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int wm = (wave_id >> 1) * 64;  // wave row offset in block tile
  const int wn = (wave_id & 1) * 64;   // wave col offset

  // staging: 128 rows x 32 k per operand; thread t loads 16 consecutive k
  // of one row (4 x float4 when fully in range)
  const int sr = threadIdx.x / 2;         // staged row 0..127
  const int sk = (threadIdx.x % 2) * 16;  // staged k 0 or 16

  f32x16 acc[2][2] = {};
  auto stage = [&](int buf, int32_t k0) {
    const int64_t xm = m0 + sr;
    const int64_t yn = n0 + sr;
    if (xm < M && yn < N && k0 + sk + 16 <= K) {
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const float4 vx = *(const float4*)&X[xm * K + k0 + sk + 4 * t];
        const float4 vy = *(const float4*)&Y[yn * K + k0 + sk + 4 * t];
        *(float4*)&lx[buf][sr][sk + 4 * t] = vx;
        *(float4*)&ly[buf][sr][sk + 4 * t] = vy;
      }
    } else {  // edge tile: element-wise with zero padding
#pragma unroll
      for (int t = 0; t < 16; t++) {
        const int32_t k = k0 + sk + t;
        lx[buf][sr][sk + t] = (xm < M && k < K) ? X[xm * K + k] : 0.f;
        ly[buf][sr][sk + t] = (yn < N && k < K) ? Y[yn * K + k] : 0.f;
      }
    }
  };
  auto compute = [&](int buf) {
    const int al = lane & 31;   // row/col within a 32-wide fragment
    const int kh = (lane >> 5); // k half within each k-pair
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; i++) {
        a[i] = lx[buf][wm + 32 * i + al][kk + kh];
        b[i] = ly[buf][wn + 32 * i + al][kk + kh];
      }
#pragma unroll
      for (int mi = 0; mi < 2; mi++)
#pragma unroll
        for (int ni = 0; ni < 2; ni++)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(
              a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
  };

  stage(0, 0);
  int buf = 0;
  for (int32_t k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();
    if (k0 + BK < K) stage(buf ^ 1, k0 + BK);
    compute(buf);
    buf ^= 1;
    __syncthreads();
  }
  // C/D layout for 32x32 f32 MFMA: col = lane&31,
  // row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)   (cdna_hip_programming.md §3)
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int ni = 0; ni < 2; ni++)
#pragma unroll
      for (int reg = 0; reg < 16; reg++) {
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        const int64_t cm = m0 + wm + 32 * mi + row;
        const int64_t cn = n0 + wn + 32 * ni + (lane & 31);
        if (cm < M && cn < N) C[cm * ldc + cn] = acc[mi][ni][reg];
      }
}

// ---------- k-means / finalize helpers ----------
__global__ void k_hist_assign(const int32_t* __restrict__ assign, int64_t n,
                              int32_t* __restrict__ counts) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&counts[assign[i]], 1);
}

__global__ void k_init_cursors(const int64_t* __restrict__ offsets, int32_t n,
                               int32_t* __restrict__ cursors) {
  int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cursors[i] = (int32_t)offsets[i];
}

__global__ void k_scatter_perm(const int32_t* __restrict__ assign, int64_t n,
                               int32_t* __restrict__ cursors,
                               uint32_t* __restrict__ perm) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  perm[i] = (uint32_t)atomicAdd(&cursors[assign[i]], 1);
}

// one list (the Flat kinds): rows keep arrival order.  The atomic cursor of
// k_scatter_perm would hand them out in whatever order the waves arrive, and
// equal distances resolve toward the smaller internal row.
__global__ void k_identity_perm(int64_t n, uint32_t* __restrict__ perm) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) perm[i] = (uint32_t)i;
}

__global__ void k_gather_rows(const float* __restrict__ src,
                              const uint32_t* __restrict__ perm, int64_t n,
                              int32_t d, float* __restrict__ dst) {
  // wave per row: dst[perm[i]] = src[i]
  int64_t i = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  if (i >= n) return;
  if (d & 3) {  // PQ subspaces of dsub % 4 != 0: rows are not 16 B aligned
    const float* s1 = src + (size_t)i * d;
    float* t1 = dst + (size_t)perm[i] * d;
    for (int j = lane; j < d; j += WAVE) t1[j] = s1[j];
    return;
  }
  const float4* s = (const float4*)(src + (size_t)i * d);
  float4* t = (float4*)(dst + (size_t)perm[i] * d);
  for (int j = lane; j < d / 4; j += WAVE) t[j] = s[j];
}

__global__ void k_gather_ids(const int64_t* __restrict__ src,
                             const uint32_t* __restrict__ perm, int64_t n,
                             int64_t* __restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[perm[i]] = src[i];
}

__global__ void k_cluster_means(const float* __restrict__ grouped,
                                const int64_t* __restrict__ offsets,
                                int32_t d, float* __restrict__ centroids) {
  // block per cluster; thread t owns dims t, t+256, ...
  // acc sized for d <= 8192 at blockDim 256 (the create-time ceiling;
  // acc[8] overflowed for IVF-PQ trains with d > 2048)
  int32_t c = blockIdx.x;
  int64_t s = offsets[c], e = offsets[c + 1];
  if (e <= s) return;  // empty: host handles split
  double acc[32] = {0};
  int nd = (d + blockDim.x - 1) / blockDim.x;
  if (nd > 32) return;  // host enforces d <= 8192
  for (int64_t r = s; r < e; r++) {
    const float* v = grouped + (size_t)r * d;
    for (int i = 0; i < nd; i++) {
      int dim = threadIdx.x + i * blockDim.x;
      if (dim < d) acc[i] += v[dim];
    }
  }
  double inv = 1.0 / (double)(e - s);
  for (int i = 0; i < nd; i++) {
    int dim = threadIdx.x + i * blockDim.x;
    if (dim < d) centroids[(size_t)c * d + dim] = (float)(acc[i] * inv);
  }
}

// ---------- exclusive scans (small n: two-level) ----------
__global__ void k_scan_block_i32(const int32_t* in, int32_t n, int64_t* out,
                                 int64_t* block_sums) {
  __shared__ int64_t lds[256];
  int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  int64_t v = (i < n) ? in[i] : 0;
  lds[threadIdx.x] = v;
  __syncthreads();
  // inclusive scan in LDS
  for (int off = 1; off < 256; off *= 2) {
    int64_t t = (threadIdx.x >= off) ? lds[threadIdx.x - off] : 0;
    __syncthreads();
    lds[threadIdx.x] += t;
    __syncthreads();
  }
  if (i <= n) out[i] = lds[threadIdx.x] - v;  // exclusive
  if (threadIdx.x == 255) block_sums[blockIdx.x] = lds[255];
}

__global__ void k_scan_add_offsets(int64_t* out, int32_t n,
                                   const int64_t* block_sums, int32_t nblocks) {
  // single block: serial scan of block sums (nblocks small), then add
  __shared__ int64_t bs[1024];
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int b = 0; b < nblocks; b++) {
      bs[b] = run;
      run += block_sums[b];
    }
    bs[nblocks] = run;
  }
  __syncthreads();
  for (int32_t i = threadIdx.x; i <= n; i += blockDim.x)
    out[i] += bs[min(i / 256, nblocks)];
}

// i64 variant (for q_total -> q_cand_base)
__global__ void k_scan_block_i64(const int64_t* in, int64_t n, int64_t* out,
                                 int64_t* block_sums) {
  __shared__ int64_t lds[256];
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t v = (i < n) ? in[i] : 0;
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int off = 1; off < 256; off *= 2) {
    int64_t t = (threadIdx.x >= off) ? lds[threadIdx.x - off] : 0;
    __syncthreads();
    lds[threadIdx.x] += t;
    __syncthreads();
  }
  if (i <= n) out[i] = lds[threadIdx.x] - v;
  if (threadIdx.x == 255) block_sums[blockIdx.x] = lds[255];
}

// ---------- binary (Hamming) indexes ----------
// Rows, queries and centroids are bit vectors packed LSB-first into u32
// words, zero-padded to wp = ceil(d/32) words (pads XOR to zero).  Distances
// are exact integers; they travel as f32 (exact below 2^24, d <= 32768) so
// the packed-u64 selection and k_emit are shared with the float indexes.

// out[q][c] = popcount(X[q] ^ Y[c]); X [nq][wp], Y [cols][wp] row-major.
// Block = 256 columns (one per thread) x kHamQ queries, words in tiles of
// kHamW.  Y rows are staged through LDS (coalesced global reads, stride
// kHamW+1 so the per-thread row walk is conflict-free); the query tile is
// stored word-major so each thread reads it as wave-uniform b128 broadcasts.
// Flat 1-D grid: tile_x + nx * tile_y (the row count of an add-time
// assignment can exceed the 65535 limit of gridDim.y).
static constexpr int kHamQ = 32;
static constexpr int kHamW = 32;
// acc[j] = popcount(X[q0 + j] ^ Y[c0 + tid]) for the block's 256 columns and
// kHamQ queries; rows and queries past the end read as zero words.  Shared
// by k_hamming_dists and k_hamming_range.
__device__ __forceinline__ void hamming_tile_acc(
    const uint32_t* __restrict__ X, int64_t nq, const uint32_t* __restrict__ Y,
    int64_t cols, int32_t wp, int64_t c0, int64_t q0, uint32_t* ly,
    uint32_t* lx, int32_t (&acc)[kHamQ]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < kHamQ; j++) acc[j] = 0;
  for (int32_t w0 = 0; w0 < wp; w0 += kHamW) {
    __syncthreads();
    for (int i = tid; i < 256 * kHamW; i += 256) {
      const int r = i / kHamW, w = i % kHamW;
      ly[r * (kHamW + 1) + w] =
          (c0 + r < cols && w0 + w < wp) ? Y[(size_t)(c0 + r) * wp + w0 + w]
                                         : 0u;
    }
    for (int i = tid; i < kHamQ * kHamW; i += 256) {
      const int q = i / kHamW, w = i % kHamW;
      lx[w * kHamQ + q] =
          (q0 + q < nq && w0 + w < wp) ? X[(size_t)(q0 + q) * wp + w0 + w]
                                       : 0u;
    }
    __syncthreads();
    const int32_t wn = min(kHamW, wp - w0);
    for (int32_t w = 0; w < wn; w++) {
      const uint32_t y = ly[tid * (kHamW + 1) + w];
      const uint4* xv = (const uint4*)(lx + w * kHamQ);
#pragma unroll
      for (int j4 = 0; j4 < kHamQ / 4; j4++) {
        const uint4 x = xv[j4];
        acc[4 * j4 + 0] += __popc(y ^ x.x);
        acc[4 * j4 + 1] += __popc(y ^ x.y);
        acc[4 * j4 + 2] += __popc(y ^ x.z);
        acc[4 * j4 + 3] += __popc(y ^ x.w);
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_hamming_dists(
    const uint32_t* __restrict__ X, int64_t nq, const uint32_t* __restrict__ Y,
    int64_t cols, int32_t wp, uint32_t nx, float* __restrict__ out,
    int64_t ld) {
  __shared__ uint32_t ly[256 * (kHamW + 1)];
  __shared__ __attribute__((aligned(16))) uint32_t lx[kHamW * kHamQ];
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)(blockIdx.x % nx) * 256;
  const int64_t q0 = (int64_t)(blockIdx.x / nx) * kHamQ;
  int32_t acc[kHamQ];
  hamming_tile_acc(X, nq, Y, cols, wp, c0, q0, ly, lx, acc);
  if (c0 + tid >= cols) return;
#pragma unroll
  for (int j = 0; j < kHamQ; j++)
    if (q0 + j < nq) out[(q0 + j) * ld + c0 + tid] = (float)acc[j];
}

// Binary Flat range search: the distance tile of k_hamming_dists with the
// radius test fused in, so no nq x N matrix is written or read back.  Run
// twice over the same inputs: the COUNT pass adds each query's hits to
// counts[q] (ballot popcount per wave, the four waves summed through LDS,
// one atomic per (block, query) with hits), the host turns counts into
// lims, and the COMPACT pass appends pack_cand(distance, row) behind
// lims[q] with one cursor atomic per (wave, query) that has hits.  A hit
// is: column in range, pass-bitmap bit set (bitmap indexed by col_base +
// column; null = every row passes), distance < radius.  Every lane takes
// part in every ballot; lanes past cols carry hit = false.  The order of a
// query's results is arbitrary (the host sorts them).
template <bool COMPACT>
__global__ void __launch_bounds__(256) k_hamming_range(
    const uint32_t* __restrict__ X, int64_t nq, const uint32_t* __restrict__ Y,
    int64_t cols, int32_t wp, uint32_t nx, int64_t col_base,
    const uint32_t* __restrict__ bitmap, int32_t radius,
    int64_t* __restrict__ counts, const int64_t* __restrict__ lims,
    int64_t* __restrict__ cursors, uint64_t* __restrict__ out) {
  __shared__ uint32_t ly[256 * (kHamW + 1)];
  __shared__ __attribute__((aligned(16))) uint32_t lx[kHamW * kHamQ];
  __shared__ int32_t lcnt[4][kHamQ];
  const int tid = threadIdx.x;
  const int lane = tid % WAVE, wave = tid / WAVE;
  const int64_t c0 = (int64_t)(blockIdx.x % nx) * 256;
  const int64_t q0 = (int64_t)(blockIdx.x / nx) * kHamQ;
  int32_t acc[kHamQ];
  hamming_tile_acc(X, nq, Y, cols, wp, c0, q0, ly, lx, acc);
  const int64_t row = col_base + c0 + tid;
  const bool ok = c0 + tid < cols &&
                  (!bitmap || ((bitmap[row >> 5] >> (row & 31)) & 1));
  if (!COMPACT) {
#pragma unroll
    for (int j = 0; j < kHamQ; j++) {
      const uint64_t b = __ballot(ok && acc[j] < radius);
      if (lane == 0) lcnt[wave][j] = __popcll(b);
    }
    __syncthreads();
    if (tid < kHamQ && q0 + tid < nq) {
      const int32_t c =
          lcnt[0][tid] + lcnt[1][tid] + lcnt[2][tid] + lcnt[3][tid];
      if (c)
        atomicAdd((unsigned long long*)&counts[q0 + tid],
                  (unsigned long long)c);
    }
  } else {
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int j = 0; j < kHamQ; j++) {
      const bool hit = ok && q0 + j < nq && acc[j] < radius;
      const uint64_t b = __ballot(hit);
      if (!b) continue;  // wave-uniform
      long long base = 0;
      if (lane == 0)
        base = (long long)atomicAdd((unsigned long long*)&cursors[q0 + j],
                                    (unsigned long long)__popcll(b));
      base = __shfl(base, 0, WAVE);
      if (hit)
        out[lims[q0 + j] + base + __popcll(b & below)] =
            pack_cand((float)acc[j], (uint32_t)row);
    }
  }
}

// argmin over a dense score row, key = score as is; tie: smaller column
__global__ void k_argmin_score(const float* __restrict__ scores, int64_t n,
                               int32_t cols, int32_t* __restrict__ out) {
  int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  if (row >= n) return;
  const float* sr = scores + row * cols;
  uint64_t best = kCandEmpty;
  for (int l = lane; l < cols; l += WAVE)
    best = min(best, pack_cand(sr[l], (uint32_t)l));
  for (int off = 32; off; off >>= 1)
    best = min(best, (uint64_t)__shfl_xor((long long)best, off, WAVE));
  if (lane == 0) out[row] = (int32_t)(best & 0xffffffffu);
}

// THE binary scan: unit = (list, 1024-row chunk) in the word-major chunk
// layout [wp][nrows_pad] u32.  Each thread owns 4 consecutive rows, so every
// word step is one coalesced 16 B/lane load and there is no cross-lane
// reduction.  The queries probing the list are staged in LDS QT at a time,
// word-major, and read as wave-uniform b128 broadcasts; per (row, query)
// pair a word costs one XOR and one accumulating popcount.  Writes the
// store-all candidates exactly like k_ivfpq_scan (key = f32 distance).
template <int QT>
__global__ void __launch_bounds__(256) k_bivf_scan(
    const uint32_t* __restrict__ units, const int64_t* __restrict__ csr_offsets,
    const int32_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_base,
    const uint32_t* __restrict__ twords, const uint32_t* __restrict__ queries,
    int32_t wp, const int32_t* __restrict__ inv_offsets,
    const int32_t* __restrict__ inv_q, const int32_t* __restrict__ inv_rank,
    const int64_t* __restrict__ qp_off, const int64_t* __restrict__ q_cand_base,
    int32_t nprobe, const uint32_t* __restrict__ bitmap, int32_t chunk_rows,
    uint64_t* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_q[];  // [wp][QT]
  __shared__ int64_t lds_cb[QT];
  const uint32_t list = units[2 * blockIdx.x];
  const uint32_t chunk = units[2 * blockIdx.x + 1];
  const int32_t iq0 = inv_offsets[list];
  const int32_t nql = inv_offsets[list + 1] - iq0;
  if (nql == 0) return;  // unprobed list (all-chunks launch)
  const int64_t list_start = csr_offsets[list];
  const int64_t len = csr_offsets[list + 1] - list_start;
  const int32_t nrows =
      (int32_t)min((int64_t)chunk_rows, len - (int64_t)chunk * chunk_rows);
  const int32_t pad = (nrows + 3) & ~3;
  const int64_t row_start = list_start + (int64_t)chunk * chunk_rows;
  const int tid = threadIdx.x;
  const int32_t r0 = 4 * tid;
  const bool active = r0 < pad;
  const uint32_t* src =
      twords + chunk_base[chunk_off[list] + (int32_t)chunk] + r0;
  uint32_t pass = 0;
  for (int i = 0; i < 4; i++) {
    const int64_t rw = row_start + r0 + i;
    if (r0 + i < nrows && (!bitmap || ((bitmap[rw >> 5] >> (rw & 31)) & 1)))
      pass |= 1u << i;
  }

  for (int32_t t0 = 0; t0 < nql; t0 += QT) {
    const int32_t qn = min(QT, nql - t0);
    __syncthreads();  // the previous tile's readers are done
    for (int32_t i = tid; i < QT * wp; i += blockDim.x) {
      const int32_t j = i / wp, w = i % wp;
      lds_q[w * QT + j] =
          j < qn ? queries[(size_t)inv_q[iq0 + t0 + j] * wp + w] : 0u;
    }
    if (tid < QT) {
      int64_t cb = 0;
      if (tid < qn) {
        const int32_t q = inv_q[iq0 + t0 + tid];
        cb = q_cand_base[q] +
             qp_off[(int64_t)q * nprobe + inv_rank[iq0 + t0 + tid]] -
             list_start;
      }
      lds_cb[tid] = cb;
    }
    __syncthreads();
    if (!active) continue;
    int32_t acc[QT][4];
#pragma unroll
    for (int j = 0; j < QT; j++)
      acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0;
#pragma unroll 4
    for (int32_t w = 0; w < wp; w++) {
      const uint4 r = *(const uint4*)(src + (size_t)w * pad);
      const uint4* qv = (const uint4*)(lds_q + w * QT);
#pragma unroll
      for (int j4 = 0; j4 < QT / 4; j4++) {
        const uint4 qq = qv[j4];
        const uint32_t qs[4] = {qq.x, qq.y, qq.z, qq.w};
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
          acc[4 * j4 + jj][0] += __popc(r.x ^ qs[jj]);
          acc[4 * j4 + jj][1] += __popc(r.y ^ qs[jj]);
          acc[4 * j4 + jj][2] += __popc(r.z ^ qs[jj]);
          acc[4 * j4 + jj][3] += __popc(r.w ^ qs[jj]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < QT; j++) {
      if (j >= qn) break;
      uint64_t* dst = cand + lds_cb[j] + row_start + r0;
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (r0 + i < nrows)
          dst[i] = (pass >> i) & 1
                       ? pack_cand((float)acc[j][i],
                                   (uint32_t)(row_start + r0 + i))
                       : kCandEmpty;
    }
  }
}

// bits -> +-1.0f rows (k-means input of the binary train); out [n][d]
__global__ void k_bits_to_pm1(const uint32_t* __restrict__ x, int64_t n,
                              int32_t d, int32_t wp, float* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * d) return;
  const int64_t r = i / d;
  const int32_t j = (int32_t)(i % d);
  out[i] = ((x[(size_t)r * wp + (j >> 5)] >> (j & 31)) & 1) ? 1.0f : -1.0f;
}

// float centroids -> packed words, bit = (value > 0); out [n][wp]
__global__ void k_binarise(const float* __restrict__ c, int64_t n, int32_t d,
                           int32_t wp, uint32_t* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * wp) return;
  const int64_t r = i / wp;
  const int32_t w = (int32_t)(i % wp);
  uint32_t bits = 0;
  for (int b = 0; b < 32; b++) {
    const int32_t j = w * 32 + b;
    if (j < d && c[(size_t)r * d + j] > 0.f) bits |= 1u << b;
  }
  out[i] = bits;
}

// ---------- launchers ----------
namespace dgk {

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

void iota_i32(hipStream_t s, int32_t* p, int64_t n, int32_t v) {
  if (n) hipLaunchKernelGGL(k_iota_i32, dim3(ceil_div(n, 256)), dim3(256), 0, s,
                            p, n, v);
}

void row_norms(hipStream_t s, const float* x, int64_t n, int32_t d,
               float* out) {
  if (!n) return;
  int wpb = 4;
  hipLaunchKernelGGL(k_row_norms, dim3(ceil_div(n, wpb)), dim3(wpb * WAVE), 0,
                     s, x, n, d, out);
}

void normalize_rows(hipStream_t s, float* x, int64_t n, int32_t d) {
  if (!n) return;
  int wpb = 4;
  hipLaunchKernelGGL(k_normalize_rows, dim3(ceil_div(n, wpb)),
                     dim3(wpb * WAVE), 0, s, x, n, d);
}

void argmin_rows(hipStream_t s, const float* dots, const float* cnorms,
                 int64_t n, int32_t nlist, int metric, int32_t* out) {
  if (!n) return;
  int wpb = 4;
  hipLaunchKernelGGL(k_argmin_rows, dim3(ceil_div(n, wpb)), dim3(wpb * WAVE),
                     0, s, dots, cnorms, n, nlist, metric, out);
}

void build_pass_bitmap(hipStream_t s, const int64_t* ids, int64_t n,
                       const dg_dev_filter* f, uint32_t* bitmap) {
  int64_t nwords = ceil_div(n, 32);
  hipLaunchKernelGGL(k_build_pass_bitmap, dim3(ceil_div(nwords, 256)),
                     dim3(256), 0, s, ids, n, *f, bitmap);
}

// choose block size by k: 2*T*k*8 <= 128 KB dynamic LDS (measured-good on
// gfx950).  Blocks shrink below a wave for the rare huge-k calls — correct,
// slow, and documented; host validates k <= 2048.
static inline int select_threads(int32_t k) {
  int T = 256;  // largest block whose per-thread lists fit 128 KB LDS
  while (T > 2 && 2ull * T * k * 8 > (128u << 10)) T >>= 1;
  return T;
}

int select_dense_threads(int32_t k) { return select_threads(k); }

void select_dense(hipStream_t s, const float* scores, const float* cnorms,
                  int64_t rows, int64_t cols, int64_t ld, int32_t nseg,
                  int32_t k, int mode, const uint32_t* bitmap,
                  int64_t col_base, uint64_t* out, int64_t out_stride,
                  int64_t out_offset) {
  int T = select_threads(k);
  size_t lds = 2ull * T * k * 8;
  int64_t seg_w = (cols + nseg - 1) / nseg;
  hipLaunchKernelGGL(k_select_dense, dim3((uint32_t)rows, (uint32_t)nseg),
                     dim3(T), lds, s, scores, cnorms, rows, cols, ld, seg_w,
                     k, mode, bitmap, col_base, out, out_stride, out_offset);
}

void select_u64(hipStream_t s, const uint64_t* cand, const int64_t* base,
                const int64_t* total, int64_t nq, int32_t k, uint64_t* out,
                int64_t out_stride) {
  int T = select_threads(k);
  size_t lds = 2ull * T * k * 8;
  hipLaunchKernelGGL(k_select_u64, dim3((uint32_t)nq), dim3(T), lds, s, cand,
                     base, total, (int64_t)-1, nq, k, out, out_stride);
}

void select_u64_uniform(hipStream_t s, const uint64_t* cand, int64_t len,
                        int64_t nq, int32_t k, uint64_t* out,
                        int64_t out_stride) {
  int T = select_threads(k);
  size_t lds = 2ull * T * k * 8;
  hipLaunchKernelGGL(k_select_u64, dim3((uint32_t)nq), dim3(T), lds, s, cand,
                     (const int64_t*)nullptr, (const int64_t*)nullptr, len,
                     nq, k, out, out_stride);
}

void coarse_select(hipStream_t s, const float* dots, const float* cnorms,
                   int64_t nq, int32_t nlist, int32_t np, int mode,
                   const uint8_t* mask, int32_t* probes, int32_t* counts) {
  hipLaunchKernelGGL(k_coarse_select, dim3((uint32_t)nq),
                     dim3(kCoarseWaveThreads), 0, s, dots, cnorms, nlist, np,
                     mode, mask, probes, counts);
}

void inv_offsets(hipStream_t s, const int32_t* counts, int32_t nlist,
                 int64_t* off64, int32_t* off32, int32_t* cursors) {
  hipLaunchKernelGGL(k_inv_offsets, dim3(1), dim3(kInvOffsetsThreads), 0, s,
                     counts, nlist, off64, off32, cursors);
}

void emit_results(hipStream_t s, const uint64_t* topk,
                  const int64_t* ids_lookup, const float* qnorms, int64_t nq,
                  int32_t k, int metric, int add_qnorm, float* out_dist,
                  int64_t* out_ids) {
  hipLaunchKernelGGL(k_emit, dim3(ceil_div(nq * k, 256)), dim3(256), 0, s,
                     topk, ids_lookup, qnorms, nq, k, metric, add_qnorm,
                     out_dist, out_ids);
}

void merge_lists(hipStream_t s, const float* dists, const int64_t* ids,
                 int32_t n_lists, int64_t nq, int32_t k_in, int32_t k_out,
                 int metric, float* out_dist, int64_t* out_ids) {
  hipLaunchKernelGGL(k_merge_lists,
                     dim3(ceil_div(nq * n_lists * k_in, 256)), dim3(256), 0,
                     s, dists, ids, n_lists, nq, k_in, k_out, (int32_t)metric,
                     out_dist, out_ids);
}

void probes_all(hipStream_t s, int64_t nq, int32_t nprobe,
                const uint8_t* mask, int32_t* probes) {
  hipLaunchKernelGGL(k_probes_all, dim3(ceil_div(nq * nprobe, 256)),
                     dim3(256), 0, s, nq, nprobe, mask, probes);
}

void probe_unpack(hipStream_t s, const uint64_t* topk, int64_t nq,
                  int32_t nprobe, const uint8_t* mask, int32_t* probes) {
  hipLaunchKernelGGL(k_probe_unpack, dim3(ceil_div(nq * nprobe, 256)),
                     dim3(256), 0, s, topk, nq, nprobe, mask, probes);
}

void hist_probes(hipStream_t s, const int32_t* probes, int64_t nq,
                 int32_t nprobe, int32_t nlist, int32_t* counts) {
  hipLaunchKernelGGL(k_hist_probes, dim3(ceil_div(nq * nprobe, 256)),
                     dim3(256), 0, s, probes, nq * nprobe, counts);
}

void scatter_probes(hipStream_t s, const int32_t* probes, int64_t nq,
                    int32_t nprobe, const int32_t* /*inv_offsets*/,
                    int32_t* cursors, int32_t* inv_q, int32_t* inv_rank) {
  hipLaunchKernelGGL(k_scatter_probes, dim3(ceil_div(nq * nprobe, 256)),
                     dim3(256), 0, s, probes, nq, nprobe, cursors, inv_q,
                     inv_rank);
}

void cand_offsets(hipStream_t s, const int32_t* probes, int64_t nq,
                  int32_t nprobe, const int64_t* csr_offsets, int64_t* qp_off,
                  int64_t* q_total) {
  hipLaunchKernelGGL(k_cand_offsets, dim3(ceil_div(nq, 128)), dim3(128), 0, s,
                     probes, nq, nprobe, csr_offsets, qp_off, q_total);
}

void alg_bytes(hipStream_t s, const int32_t* inv_counts,
               const int64_t* csr_offsets, int32_t nlist, int64_t row_bytes,
               int64_t* out) {
  hipLaunchKernelGGL(k_alg_bytes, dim3(16), dim3(256), 0, s, inv_counts,
                     csr_offsets, nlist, row_bytes, out);
}

void fill_unit_counts(hipStream_t s, const int32_t* inv_counts, int32_t nlist,
                      const int64_t* csr_offsets, int32_t chunk_rows,
                      int32_t* unit_counts) {
  hipLaunchKernelGGL(k_unit_counts, dim3(ceil_div(nlist, 128)), dim3(128), 0,
                     s, inv_counts, nlist, csr_offsets, chunk_rows,
                     unit_counts);
}

void fill_units(hipStream_t s, const int32_t* unit_offsets,
                const int32_t* unit_counts, int32_t nlist,
                const int64_t* /*csr_offsets*/, int32_t /*chunk_rows*/,
                uint32_t* units, int32_t /*total*/) {
  hipLaunchKernelGGL(k_fill_units, dim3(ceil_div(nlist, 128)), dim3(128), 0,
                     s, unit_offsets, unit_counts, nlist, units);
}

void ivf_scan_col(hipStream_t s, const uint32_t* units, int32_t n_units,
                  const int64_t* csr_offsets, const int32_t* chunk_off,
                  const int64_t* chunk_base, const float* tvec,
                  const float* vnorms, const float* queries, int32_t d,
                  const int32_t* inv_offsets, const int32_t* inv_q,
                  const int32_t* inv_rank, const int64_t* qp_off,
                  const int64_t* q_cand_base, int32_t nprobe, int metric,
                  const uint32_t* bitmap, int32_t chunk_rows,
                  uint64_t* cand, int32_t mean_probes) {
  if (!n_units) return;
  static int variant = []() {
    const char* e = getenv("DG_SCAN_VARIANT");
    return e ? atoi(e) : 0;
  }();
#define DG_SCAN_LAUNCH(QTM, RPL)                                            \
  do {                                                                      \
    size_t lds = (size_t)(QTM) * d * 4 + (QTM) * 8;                         \
    hipLaunchKernelGGL((k_ivf_scan_col<(QTM), (RPL)>),                      \
                       dim3((uint32_t)n_units), dim3(256), lds, s, units,   \
                       csr_offsets, chunk_off, chunk_base, tvec, vnorms,    \
                       queries, d, inv_offsets, inv_q, inv_rank, qp_off,    \
                       q_cand_base, nprobe, metric, bitmap, chunk_rows,     \
                       cand);                                               \
  } while (0)
  switch (variant) {
    case 1: DG_SCAN_LAUNCH(8, 4); break;
    case 2: DG_SCAN_LAUNCH(16, 2); break;
    case 3: DG_SCAN_LAUNCH(8, 8); break;
    case 4: DG_SCAN_LAUNCH(4, 4); break;
    case 5: DG_SCAN_LAUNCH(12, 4); break;
    case 8: {
      constexpr int QTM = 16;
      size_t lds = (size_t)QTM * d * 4 + QTM * 8;
      hipLaunchKernelGGL((k_ivf_scan_col_nt<QTM, 4>),
                         dim3((uint32_t)n_units), dim3(256), lds, s, units,
                         csr_offsets, chunk_off, chunk_base, tvec, vnorms,
                         queries, d, inv_offsets, inv_q, inv_rank, qp_off,
                         q_cand_base, nprobe, metric, bitmap, chunk_rows,
                         cand);
      break;
    }
    case 7: {
      constexpr int QTM = 16, DEPTH = 6;
      size_t lds = (size_t)QTM * d * 4 + 4 * DEPTH * 4 * 256 * 4 + QTM * 8;
      hipLaunchKernelGGL((k_ivf_scan_glds<QTM, DEPTH>),
                         dim3((uint32_t)n_units), dim3(256), lds, s, units,
                         csr_offsets, chunk_off, chunk_base, tvec, vnorms,
                         queries, d, inv_offsets, inv_q, inv_rank, qp_off,
                         q_cand_base, nprobe, metric, bitmap, chunk_rows,
                         cand);
      break;
    }
    case 6: {
      constexpr int QTM = 16;
      size_t lds = (size_t)QTM * d * 4 + QTM * 8;
      hipLaunchKernelGGL((k_ivf_scan_col_hi<QTM, 4>),
                         dim3((uint32_t)n_units), dim3(256), lds, s, units,
                         csr_offsets, chunk_off, chunk_base, tvec, vnorms,
                         queries, d, inv_offsets, inv_q, inv_rank, qp_off,
                         q_cand_base, nprobe, metric, bitmap, chunk_rows,
                         cand);
      break;
    }
    case 0:
    case 12: {  // DEFAULT (round 2): asm-load pipeline with full-drain
      // waits — the counted-wait variants (10/13/14) are faster on paper
      // but LLVM's allocator cannot be made to respect in-flight asm-load
      // destinations (verified by static hazard scan + GPU faults); the
      // drain form is airtight and measured fastest of the correct set.
      // QTM shrinks for large d so the query tile fits the 160 KB LDS.
#define DG_PIPE_LAUNCH(QTM)                                                 \
  do {                                                                      \
    size_t lds = (size_t)(QTM) * d * 4 + (QTM) * 8;                         \
    hipLaunchKernelGGL((k_ivf_scan_pipe<(QTM), true>),                      \
                       dim3((uint32_t)n_units), dim3(256), lds, s, units,   \
                       csr_offsets, chunk_off, chunk_base, tvec, vnorms,    \
                       queries, d, inv_offsets, inv_q, inv_rank, qp_off,    \
                       q_cand_base, nprobe, metric, bitmap, chunk_rows,     \
                       cand, 0, 0);                                         \
  } while (0)
      (void)mean_probes;  // dense-batch 20/24-query tiles fail the
                          // in-flight hazard scan (allocator stashes
                          // pending asm loads at >=250 VGPRs) — QTM=16
                          // is the largest clean tile
      if (d <= 2304)
        DG_PIPE_LAUNCH(16);
      else if (d <= 4608)
        DG_PIPE_LAUNCH(8);
      else
        DG_PIPE_LAUNCH(4);  // d <= 8192 (create-time cap)
#undef DG_PIPE_LAUNCH
      break;
    }
    // (case 19 pipe4 removed: 2x8-bank wait/issue/compute order also
    // fails the hazard scan — 8 pending loads across a full compute push
    // the allocator into stashing in-flight destinations)
    case 15: {  // round-1 columnar pipeline (previous default)
      DG_SCAN_LAUNCH(16, 4);
      break;
    }
// (pipe2/pipe3 launch cases removed: every counted-wait or batched-issue
// schedule fails the static in-flight-register hazard scan — kernels kept
// above as the documented record of the attempt)
    case 9: {  // (12,4) capped to 3 waves/SIMD (uncapped allocates 177)
      constexpr int QTM = 12;
      size_t lds = (size_t)QTM * d * 4 + QTM * 8;
      hipLaunchKernelGGL((k_ivf_scan_col_hi<QTM, 4>),
                         dim3((uint32_t)n_units), dim3(256), lds, s, units,
                         csr_offsets, chunk_off, chunk_base, tvec, vnorms,
                         queries, d, inv_offsets, inv_q, inv_rank, qp_off,
                         q_cand_base, nprobe, metric, bitmap, chunk_rows,
                         cand);
      break;
    }
    default: DG_SCAN_LAUNCH(16, 4); break;
  }
#undef DG_SCAN_LAUNCH
}

void ivf_scan_topk(hipStream_t s, const uint32_t* units, int32_t n_units,
                   const int64_t* csr_offsets, const int32_t* chunk_off,
                   const int64_t* chunk_base, const float* tvec,
                   const float* vnorms, const float* queries, int32_t d,
                   const int32_t* inv_offsets, const int32_t* inv_q,
                   const int32_t* inv_rank, int32_t nprobe, int metric,
                   const uint32_t* bitmap, int32_t chunk_rows, int32_t k,
                   int32_t cpl_max, uint64_t* partial, bool mfma,
                   int64_t nq, float* qimage, int32_t pair_py) {
  if (!n_units) return;
  if (mfma) {
    // pair scan first (the heavy units), then the tiles it leaves
    const int32_t pairing = qimage && dg_scan_pair_applies(d, nq) ? 1 : 0;
    if (pairing) {
      const int64_t nf4 = (int64_t)((d + 15) / 16) * 4 * (nq + 1);
      hipLaunchKernelGGL(k_query_image, dim3((uint32_t)((nf4 + 255) / 256)),
                         dim3(256), 0, s, queries, nq, d, qimage);
#define DG_PAIR_LAUNCH(SHORT)                                               \
  hipLaunchKernelGGL((k_ivf_scan_mfma2<(SHORT)>),                           \
                     dim3((uint32_t)n_units, (uint32_t)pair_py), dim3(256), \
                     0, s, units, csr_offsets, chunk_off, chunk_base, tvec, \
                     vnorms, qimage, (int32_t)nq, d, inv_offsets, inv_q,    \
                     inv_rank, nprobe, metric, bitmap, chunk_rows, partial, \
                     k, cpl_max)
      if (d <= 16)
        DG_PAIR_LAUNCH(true);
      else
        DG_PAIR_LAUNCH(false);
#undef DG_PAIR_LAUNCH
    }
    // same tile ladder; the LDS image is padded to whole 16-dim periods
#define DG_MFMA_LAUNCH(QTM)                                                 \
  do {                                                                      \
    size_t lds = (size_t)((d + 15) / 16) * (QTM) * 64 + (QTM) * 8;          \
    hipLaunchKernelGGL((k_ivf_scan_mfma<(QTM)>), dim3((uint32_t)n_units),   \
                       dim3(256), lds, s, units, csr_offsets, chunk_off,    \
                       chunk_base, tvec, vnorms, queries, d, inv_offsets,   \
                       inv_q, inv_rank, nprobe, metric, bitmap, chunk_rows, \
                       partial, k, cpl_max, pairing);                       \
  } while (0)
    if (d <= 2304)
      DG_MFMA_LAUNCH(16);
    else if (d <= 4608)
      DG_MFMA_LAUNCH(8);
    else
      DG_MFMA_LAUNCH(4);
#undef DG_MFMA_LAUNCH
    return;
  }
  // same tile ladder as the default ivf_scan_col pipeline
#define DG_PIPE_LAUNCH(QTM)                                                 \
  do {                                                                      \
    size_t lds = (size_t)(QTM) * d * 4 + (QTM) * 8;                         \
    hipLaunchKernelGGL((k_ivf_scan_pipe<(QTM), true, true>),                \
                       dim3((uint32_t)n_units), dim3(256), lds, s, units,   \
                       csr_offsets, chunk_off, chunk_base, tvec, vnorms,    \
                       queries, d, inv_offsets, inv_q, inv_rank, nullptr,   \
                       nullptr, nprobe, metric, bitmap, chunk_rows,         \
                       partial, k, cpl_max);                                \
  } while (0)
  if (d <= 2304)
    DG_PIPE_LAUNCH(16);
  else if (d <= 4608)
    DG_PIPE_LAUNCH(8);
  else
    DG_PIPE_LAUNCH(4);
#undef DG_PIPE_LAUNCH
}

void ivf_scan_f16(hipStream_t s, const uint32_t* units, int32_t n_units,
                  const int64_t* csr_offsets, const int32_t* chunk_off,
                  const int64_t* chunk_base, const __half* tvec,
                  const float* vnorms, const float* queries, int32_t d,
                  const int32_t* inv_offsets, const int32_t* inv_q,
                  const int32_t* inv_rank, const int64_t* qp_off,
                  const int64_t* q_cand_base, int32_t nprobe, int metric,
                  const uint32_t* bitmap, int32_t chunk_rows, bool fused,
                  int32_t k, int32_t cpl_max, uint64_t* out, int32_t py) {
  if (!n_units) return;
  // the tile ladder of k_ivf_scan_mfma; the LDS image is padded to whole
  // 32-dim periods
#define DG_F16_LAUNCH(QTM, FUSED)                                           \
  do {                                                                      \
    size_t lds = (size_t)((d + 31) / 32) * 2 * (QTM) * 64 + (QTM) * 8;      \
    hipLaunchKernelGGL((k_ivf_scan_f16<(QTM), (FUSED)>),                    \
                       dim3((uint32_t)n_units, (uint32_t)py), dim3(256),    \
                       lds, s, units, csr_offsets, chunk_off, chunk_base,   \
                       tvec, vnorms, queries, d, inv_offsets, inv_q,        \
                       inv_rank, qp_off, q_cand_base, nprobe, metric,       \
                       bitmap, chunk_rows, out, k, cpl_max);                \
  } while (0)
#define DG_F16_LADDER(FUSED)                                                \
  do {                                                                      \
    if (d <= 2304)                                                          \
      DG_F16_LAUNCH(16, FUSED);                                             \
    else if (d <= 4608)                                                     \
      DG_F16_LAUNCH(8, FUSED);                                              \
    else                                                                    \
      DG_F16_LAUNCH(4, FUSED);                                              \
  } while (0)
  if (fused)
    DG_F16_LADDER(true);
  else
    DG_F16_LADDER(false);
#undef DG_F16_LADDER
#undef DG_F16_LAUNCH
}

void f32_to_f16_check(hipStream_t s, const float* in, int64_t n, __half* out,
                      int32_t* overflow) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_f32_to_f16_check, dim3((uint32_t)ceil_div(n, 256)),
                     dim3(256), 0, s, in, n, out, overflow);
}

void row_norms_f16(hipStream_t s, const __half* x, int64_t n, int32_t d,
                   float* out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_row_norms_f16, dim3((uint32_t)ceil_div(n, 4)),
                     dim3(256), 0, s, x, n, d, out);
}

void gather_rows_by_index_f16(hipStream_t s, const __half* src,
                              const int64_t* idx, int64_t n, int32_t d,
                              float* dst) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gather_rows_by_index_f16,
                     dim3((uint32_t)ceil_div(n * d, 256)), dim3(256), 0, s,
                     src, idx, n, d, dst);
}

void transpose_chunks_f16(hipStream_t s, const uint32_t* units,
                          int32_t n_units, const int64_t* csr_offsets,
                          const int32_t* chunk_off, const int64_t* chunk_base,
                          const __half* rowmajor, int32_t d,
                          int32_t chunk_rows, __half* tvec) {
  if (!n_units) return;
  hipLaunchKernelGGL(k_transpose_chunks_f16, dim3((uint32_t)n_units),
                     dim3(256), 0, s, units, csr_offsets, chunk_off,
                     chunk_base, rowmajor, d, chunk_rows, tvec);
}

void ivf_scan_sq8(hipStream_t s, const uint32_t* units, int32_t n_units,
                  const int64_t* csr_offsets, const int32_t* chunk_off,
                  const int64_t* chunk_base, const uint8_t* tvec,
                  const float* vnorms, const float* qprime, const float* cq,
                  int32_t d, const int32_t* inv_offsets, const int32_t* inv_q,
                  const int32_t* inv_rank, const int64_t* qp_off,
                  const int64_t* q_cand_base, int32_t nprobe, int metric,
                  const uint32_t* bitmap, int32_t chunk_rows, bool fused,
                  int32_t k, int32_t cpl_max, uint64_t* out, int32_t py) {
  if (!n_units) return;
  // the tile ladder of k_ivf_scan_mfma; the LDS image is one 16-dim period
  // per kp, then cbase and the tile's cq
#define DG_SQ8_LAUNCH(QTM, FUSED)                                           \
  do {                                                                      \
    size_t lds = (size_t)((d + 15) / 16) * (QTM) * 64 + (QTM) * 12;         \
    hipLaunchKernelGGL((k_ivf_scan_sq8<(QTM), (FUSED)>),                    \
                       dim3((uint32_t)n_units, (uint32_t)py), dim3(256),    \
                       lds, s, units, csr_offsets, chunk_off, chunk_base,   \
                       tvec, vnorms, qprime, cq, d, inv_offsets, inv_q,     \
                       inv_rank, qp_off, q_cand_base, nprobe, metric,       \
                       bitmap, chunk_rows, out, k, cpl_max);                \
  } while (0)
#define DG_SQ8_LADDER(FUSED)                                                \
  do {                                                                      \
    if (d <= 2304)                                                          \
      DG_SQ8_LAUNCH(16, FUSED);                                             \
    else if (d <= 4608)                                                     \
      DG_SQ8_LAUNCH(8, FUSED);                                              \
    else                                                                    \
      DG_SQ8_LAUNCH(4, FUSED);                                              \
  } while (0)
  if (fused)
    DG_SQ8_LADDER(true);
  else
    DG_SQ8_LADDER(false);
#undef DG_SQ8_LADDER
#undef DG_SQ8_LAUNCH
}

void sq8_encode_check(hipStream_t s, const float* in, int64_t n, int32_t d,
                      const float* vmin, const float* vdiff, uint8_t* out,
                      int32_t* bad) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sq8_encode_check, dim3((uint32_t)ceil_div(n, 256)),
                     dim3(256), 0, s, in, n, d, vmin, vdiff, out, bad);
}

void row_norms_sq8(hipStream_t s, const uint8_t* x, int64_t n, int32_t d,
                   const float* vmin, const float* vdiff, float* out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_row_norms_sq8, dim3((uint32_t)ceil_div(n, 4)),
                     dim3(256), 0, s, x, n, d, vmin, vdiff, out);
}

void gather_rows_by_index_sq8(hipStream_t s, const uint8_t* src,
                              const int64_t* idx, int64_t n, int32_t d,
                              const float* vmin, const float* vdiff,
                              float* dst) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gather_rows_by_index_sq8,
                     dim3((uint32_t)ceil_div(n * d, 256)), dim3(256), 0, s,
                     src, idx, n, d, vmin, vdiff, dst);
}

void sq8_fold_query(hipStream_t s, const float* q, int64_t nq, int32_t d,
                    const float* vmin, const float* step, float* qp,
                    float* cq) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_sq8_fold_query, dim3((uint32_t)nq), dim3(256), 0, s,
                     q, d, vmin, step, qp, cq);
}

void transpose_chunks_sq8(hipStream_t s, const uint32_t* units,
                          int32_t n_units, const int64_t* csr_offsets,
                          const int32_t* chunk_off, const int64_t* chunk_base,
                          const uint8_t* rowmajor, int32_t d,
                          int32_t chunk_rows, uint8_t* tvec) {
  if (!n_units) return;
  hipLaunchKernelGGL(k_transpose_chunks_sq8, dim3((uint32_t)n_units),
                     dim3(256), 0, s, units, csr_offsets, chunk_off,
                     chunk_base, rowmajor, d, chunk_rows, tvec);
}

// per-dimension min and max - min (f32) of x [n x d], for dg_train
__global__ void __launch_bounds__(256) k_sq8_col_minmax(
    const float* __restrict__ x, int64_t n, int32_t d,
    float* __restrict__ vmin, float* __restrict__ vdiff) {
  __shared__ float smin[256], smax[256];
  const int32_t j = blockIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t r = threadIdx.x; r < n; r += blockDim.x) {
    const float v = x[(size_t)r * d + j];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  smin[threadIdx.x] = lo;
  smax[threadIdx.x] = hi;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      smin[threadIdx.x] = fminf(smin[threadIdx.x], smin[threadIdx.x + off]);
      smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + off]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    vmin[j] = smin[0];
    vdiff[j] = smax[0] - smin[0];
  }
}

void sq8_col_minmax(hipStream_t s, const float* x, int64_t n, int32_t d,
                    float* vmin, float* vdiff) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sq8_col_minmax, dim3((uint32_t)d), dim3(256), 0, s, x,
                     n, d, vmin, vdiff);
}

void range_emit(hipStream_t s, const uint64_t* packed, const int64_t* lims,
                const int64_t* ids_lookup, const float* qnorms, int64_t nq,
                int metric, int add_qnorm, float* out_dist,
                int64_t* out_ids) {
  hipLaunchKernelGGL(k_range_emit, dim3((uint32_t)nq), dim3(256), 0, s,
                     packed, lims, ids_lookup, qnorms, nq, metric, add_qnorm,
                     out_dist, out_ids);
}

void count_below(hipStream_t s, const uint64_t* cand, const int64_t* base,
                 const int64_t* total, const uint64_t* thr, int metric,
                 const float* qnorms, float radius, int64_t nq,
                 int64_t* counts) {
  hipLaunchKernelGGL(k_count_below, dim3((uint32_t)nq), dim3(256), 0, s,
                     cand, base, total, thr, metric, qnorms, radius, nq,
                     counts);
}

void compact_below(hipStream_t s, const uint64_t* cand, const int64_t* base,
                   const int64_t* total, const uint64_t* thr, int metric,
                   const float* qnorms, float radius, const int64_t* out_off,
                   int64_t nq, int64_t* cursors, uint64_t* out) {
  hipLaunchKernelGGL(k_compact_below, dim3((uint32_t)nq), dim3(256), 0, s,
                     cand, base, total, thr, metric, qnorms, radius, out_off,
                     nq, cursors, out);
}

void count_below_dense(hipStream_t s, const float* scores,
                       const float* cnorms, int64_t rows, int64_t cols,
                       int mode, const uint32_t* bitmap, int64_t col_base,
                       const float* qnorms, float radius, int64_t* counts) {
  hipLaunchKernelGGL(k_count_below_dense, dim3((uint32_t)rows), dim3(256), 0,
                     s, scores, cnorms, rows, cols, mode, bitmap, col_base,
                     qnorms, radius, counts);
}

void compact_below_dense(hipStream_t s, const float* scores,
                         const float* cnorms, int64_t rows, int64_t cols,
                         int mode, const uint32_t* bitmap, int64_t col_base,
                         const float* qnorms, float radius,
                         const int64_t* out_off, int64_t* cursors,
                         uint64_t* out) {
  hipLaunchKernelGGL(k_compact_below_dense, dim3((uint32_t)rows), dim3(256),
                     0, s, scores, cnorms, rows, cols, mode, bitmap,
                     col_base, qnorms, radius, out_off, cursors, out);
}

void residual(hipStream_t s, const float* x, const int32_t* assign,
              const float* centroids, int64_t n, int32_t d, float* out) {
  if (n) hipLaunchKernelGGL(k_residual, dim3(ceil_div(n, 4)), dim3(4 * WAVE),
                            0, s, x, assign, centroids, n, d, out);
}

void set_code(hipStream_t s, const int32_t* amin, int64_t n, int32_t m,
              int32_t code_size, int32_t nbits, uint8_t* codes) {
  if (n) hipLaunchKernelGGL(k_set_code, dim3(ceil_div(n, 256)), dim3(256), 0,
                            s, amin, n, m, code_size, nbits, codes);
}

void gather_codes(hipStream_t s, const uint8_t* src, const uint32_t* perm,
                  int64_t n, int32_t M, uint8_t* dst) {
  if (n) hipLaunchKernelGGL(k_gather_codes, dim3(ceil_div(n, 8)),
                            dim3(8 * 32), 0, s, src, perm, n, M, dst);
}

void build_S(hipStream_t s, const float* centroids, const float* codebooks,
             int32_t nlist, int32_t M, int32_t ksub, int32_t dsub, int32_t d,
             __half* S, int32_t* overflow) {
  int64_t total = (int64_t)nlist * M * ksub;
  hipLaunchKernelGGL(k_build_S, dim3(ceil_div(total, 256)), dim3(256), 0, s,
                     centroids, codebooks, nlist, M, ksub, dsub, d, S,
                     overflow);
}

// dynamic LDS one launch may ask for on the current device (160 KiB on
// MI355X); 0 if the query fails, which rejects every IVF-PQ geometry
size_t max_launch_lds() {
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock,
                            dev) != hipSuccess ||
      v < 0)
    return 0;
  return (size_t)v;
}

// LDS of one k_ivfpq_scan block: the staged code tile + the f16 S_l table
size_t ivfpq_scan_lds(int32_t tile_rows, int32_t M) {
  return (size_t)tile_rows * M + (size_t)M * 256 * 2;
}

// LDS of one k_ivfpq4_scan block: four per-wave f32 lookup tables, the f16
// S_l table and the packed code tile with its odd dword row stride
size_t ivfpq4_scan_lds(int32_t M) {
  return (size_t)4 * M * 16 * 4 + (size_t)M * 16 * 2 +
         (size_t)kPqTileRows * pq4_row_stride(M) * 4;
}

void f32_to_f16(hipStream_t s, const float* in, int64_t n, __half* out) {
  if (n) hipLaunchKernelGGL(k_f32_to_f16, dim3(ceil_div(n, 256)), dim3(256),
                            0, s, in, n, out);
}

hipError_t ivfpq_scan(hipStream_t s, const uint32_t* units, int32_t n_units,
                      const int64_t* csr_offsets, const uint8_t* csr_codes,
                      const __half* S, const __half* T,
                      const float* coarse_dots, int32_t nlist, int32_t M,
                      const int32_t* inv_offsets, const int32_t* inv_q,
                      const int32_t* inv_rank, const int64_t* qp_off,
                      const int64_t* q_cand_base, int32_t nprobe, int metric,
                      const uint32_t* bitmap, int32_t chunk_rows,
                      uint64_t* cand, int32_t nbits) {
  if (!n_units) return hipSuccess;
  if (nbits == 4) {
    const size_t lds4 = ivfpq4_scan_lds(M);
    if (lds4 > max_launch_lds()) return hipErrorInvalidValue;  // no launch
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ivfpq4_scan, dim3((uint32_t)n_units), dim3(256),
                       lds4, s, units, csr_offsets, csr_codes, S, T,
                       coarse_dots, nlist, M, inv_offsets, inv_q, inv_rank,
                       qp_off, q_cand_base, nprobe, metric, bitmap,
                       chunk_rows, cand);
    return hipGetLastError();
  }
  if (nbits != 8) return hipErrorInvalidValue;
  // T-table (L2/L3) traffic per chunk scales as 1/TILE: every staged tile
  // walks each probing query's 48 KB T window once, so the largest tile
  // whose codes + S_l fit LDS wins unless occupancy dominates (A/B'd;
  // DG_PQ_RPV forces a tile for experiments).  TILE = RPV * 64 rows.
  const char* e = getenv("DG_PQ_RPV");
  int rpv = e ? atoi(e) : 4;  // 256-row tiles + 2 blocks/CU measured best
  if (rpv != 4 && rpv != 6 && rpv != 8 && rpv != 16 && rpv != 17) rpv = 4;
  auto tile_lds = [&](int r) {
    return ivfpq_scan_lds((r == 6 ? 4 : (r == 17 ? 16 : r)) * WAVE, M);
  };
  // a forced tile that does not fit falls back to the default one, whose
  // fit dg_index_create has checked (kPqTileRows)
  const size_t lds_max = max_launch_lds();
  if (tile_lds(rpv) > lds_max) rpv = 4;
  const size_t lds = tile_lds(rpv);
  if (lds > lds_max) return hipErrorInvalidValue;  // never issue the launch
  (void)hipGetLastError();  // the status read below is this launch's own
  if (rpv == 17) {  // cooperative: 4 waves share each query's T window
    hipLaunchKernelGGL((k_ivfpq_scan<16, 1, true>), dim3((uint32_t)n_units),
                       dim3(256), lds, s, units, csr_offsets, csr_codes, S,
                       T, coarse_dots, nlist, M, inv_offsets, inv_q,
                       inv_rank, qp_off, q_cand_base, nprobe, metric, bitmap,
                       chunk_rows, cand);
    return hipGetLastError();
  }
  if (rpv == 6)  // round-1 form: VGPRs capped at 80 by launch_bounds(256,6)
    hipLaunchKernelGGL((k_ivfpq_scan<4, 6>), dim3((uint32_t)n_units),
                       dim3(256), lds, s, units, csr_offsets, csr_codes, S,
                       T, coarse_dots, nlist, M, inv_offsets, inv_q,
                       inv_rank, qp_off, q_cand_base, nprobe, metric, bitmap,
                       chunk_rows, cand);
  else if (rpv == 16)
    hipLaunchKernelGGL((k_ivfpq_scan<16, 1>), dim3((uint32_t)n_units), dim3(256),
                       lds, s, units, csr_offsets, csr_codes, S, T,
                       coarse_dots, nlist, M, inv_offsets, inv_q, inv_rank,
                       qp_off, q_cand_base, nprobe, metric, bitmap,
                       chunk_rows, cand);
  else if (rpv == 8)
    hipLaunchKernelGGL((k_ivfpq_scan<8, 1>), dim3((uint32_t)n_units), dim3(256),
                       lds, s, units, csr_offsets, csr_codes, S, T,
                       coarse_dots, nlist, M, inv_offsets, inv_q, inv_rank,
                       qp_off, q_cand_base, nprobe, metric, bitmap,
                       chunk_rows, cand);
  else  // default: 256-row tiles with the register cap lifted (2 blocks/CU
        // by LDS anyway; 80-VGPR cap limited outstanding T gathers)
    hipLaunchKernelGGL((k_ivfpq_scan<4, 2>), dim3((uint32_t)n_units),
                       dim3(256), lds, s, units, csr_offsets, csr_codes, S,
                       T, coarse_dots, nlist, M, inv_offsets, inv_q,
                       inv_rank, qp_off, q_cand_base, nprobe, metric, bitmap,
                       chunk_rows, cand);
  return hipGetLastError();
}

void transpose_chunks(hipStream_t s, const uint32_t* units, int32_t n_units,
                      const int64_t* csr_offsets, const int32_t* chunk_off,
                      const int64_t* chunk_base, const float* rowmajor,
                      int32_t d, int32_t chunk_rows, float* tvec) {
  if (!n_units) return;
  hipLaunchKernelGGL(k_transpose_chunks<float>, dim3((uint32_t)n_units),
                     dim3(256), 0, s, units, csr_offsets, chunk_off,
                     chunk_base, rowmajor, d, chunk_rows, tvec);
}

void transpose_chunks_u32(hipStream_t s, const uint32_t* units,
                          int32_t n_units, const int64_t* csr_offsets,
                          const int32_t* chunk_off, const int64_t* chunk_base,
                          const uint32_t* rowmajor, int32_t wp,
                          int32_t chunk_rows, uint32_t* twords) {
  if (!n_units) return;
  hipLaunchKernelGGL(k_transpose_chunks<uint32_t>, dim3((uint32_t)n_units),
                     dim3(256), 0, s, units, csr_offsets, chunk_off,
                     chunk_base, rowmajor, wp, chunk_rows, twords);
}

void dots_mfma(hipStream_t s, const float* X, int64_t M, const float* Y,
               int64_t N, int32_t K, float* C, int64_t ldc) {
  dim3 grid((uint32_t)((N + 127) / 128), (uint32_t)((M + 127) / 128));
  hipLaunchKernelGGL(k_dots_mfma, grid, dim3(256), 0, s, X, Y, M, N, K, C,
                     ldc);
}

void hist_assign(hipStream_t s, const int32_t* assign, int64_t n,
                 int32_t nlist, int32_t* counts) {
  hipLaunchKernelGGL(k_hist_assign, dim3(ceil_div(n, 256)), dim3(256), 0, s,
                     assign, n, counts);
}

void init_cursors(hipStream_t s, const int64_t* offsets, int32_t n,
                  int32_t* cursors) {
  hipLaunchKernelGGL(k_init_cursors, dim3(ceil_div(n, 128)), dim3(128), 0, s,
                     offsets, n, cursors);
}

void scatter_perm(hipStream_t s, const int32_t* assign, int64_t n,
                  const int64_t* /*offsets*/, int32_t* cursors,
                  uint32_t* perm) {
  hipLaunchKernelGGL(k_scatter_perm, dim3(ceil_div(n, 256)), dim3(256), 0, s,
                     assign, n, cursors, perm);
}

void identity_perm(hipStream_t s, int64_t n, uint32_t* perm) {
  hipLaunchKernelGGL(k_identity_perm, dim3(ceil_div(n, 256)), dim3(256), 0, s,
                     n, perm);
}

void gather_rows(hipStream_t s, const float* src, const uint32_t* perm,
                 int64_t n, int32_t d, float* dst) {
  if (!n) return;
  int wpb = 4;
  hipLaunchKernelGGL(k_gather_rows, dim3(ceil_div(n, wpb)), dim3(wpb * WAVE),
                     0, s, src, perm, n, d, dst);
}

void gather_ids(hipStream_t s, const int64_t* src, const uint32_t* perm,
                int64_t n, int64_t* dst) {
  hipLaunchKernelGGL(k_gather_ids, dim3(ceil_div(n, 256)), dim3(256), 0, s,
                     src, perm, n, dst);
}

void cluster_means(hipStream_t s, const float* grouped, const int64_t* offsets,
                   int32_t nlist, int32_t d, float* centroids) {
  hipLaunchKernelGGL(k_cluster_means, dim3(nlist), dim3(256), 0, s, grouped,
                     offsets, d, centroids);
}

void excl_scan_i32_to_i64(hipStream_t s, const int32_t* in, int32_t n,
                          int64_t* out, int64_t* bs) {
  int nblocks = (int)ceil_div(n + 1, 256);  // thread i==n writes the total
  hipLaunchKernelGGL(k_scan_block_i32, dim3(nblocks), dim3(256), 0, s, in, n,
                     out, bs);
  hipLaunchKernelGGL(k_scan_add_offsets, dim3(1), dim3(256), 0, s, out, n, bs,
                     nblocks);
}

void excl_scan_i64(hipStream_t s, const int64_t* in, int64_t n, int64_t* out,
                   int64_t* bs) {
  int nblocks = (int)ceil_div(n + 1, 256);
  hipLaunchKernelGGL(k_scan_block_i64, dim3(nblocks), dim3(256), 0, s, in, n,
                     out, bs);
  hipLaunchKernelGGL(k_scan_add_offsets, dim3(1), dim3(256), 0, s, out,
                     (int32_t)n, bs, nblocks);
}

void gather_rows_by_index(hipStream_t s, const float* src, const int64_t* idx,
                          int64_t n, int32_t d, float* dst) {
  if (!n) return;
  hipLaunchKernelGGL(k_gather_rows_by_index, dim3(ceil_div(n, 4)),
                     dim3(4 * WAVE), 0, s, src, idx, n, d, dst);
}

void fill_base_total(hipStream_t s, int64_t nq, int64_t len, int64_t* base,
                     int64_t* total) {
  hipLaunchKernelGGL(k_fill_base_total, dim3(ceil_div(nq, 256)), dim3(256), 0,
                     s, nq, len, base, total);
}

void tombstone(hipStream_t s, const int64_t* pos, int64_t n, int64_t* ids) {
  if (n) hipLaunchKernelGGL(k_tombstone, dim3(ceil_div(n, 256)), dim3(256), 0,
                            s, pos, n, ids);
}

// ---- binary (Hamming) indexes ----
void hamming_dists(hipStream_t s, const uint32_t* X, int64_t nq,
                   const uint32_t* Y, int64_t cols, int32_t wp, float* out,
                   int64_t ld) {
  if (!nq || !cols) return;
  const int64_t nx = ceil_div(cols, 256), ny = ceil_div(nq, kHamQ);
  hipLaunchKernelGGL(k_hamming_dists, dim3((uint32_t)(nx * ny)), dim3(256), 0,
                     s, X, nq, Y, cols, wp, (uint32_t)nx, out, ld);
}

void hamming_range(hipStream_t s, bool compact, const uint32_t* X, int64_t nq,
                   const uint32_t* Y, int64_t cols, int32_t wp,
                   const uint32_t* bitmap, int32_t radius, int64_t* counts,
                   const int64_t* lims, int64_t* cursors, uint64_t* out,
                   int64_t max_blocks) {
  if (!nq || !cols) return;
  const int64_t ny = ceil_div(nq, kHamQ);
  // column spans keep the 1-D grid at max_blocks (at least one column tile)
  const int64_t tiles = max_blocks / ny;
  const int64_t span = (tiles > 0 ? tiles : 1) * 256;
  for (int64_t cb = 0; cb < cols; cb += span) {
    const int64_t cc = cols - cb < span ? cols - cb : span;
    const int64_t nx = ceil_div(cc, 256);
    const uint32_t* Yc = Y + (size_t)cb * wp;
    if (compact)
      hipLaunchKernelGGL(k_hamming_range<true>, dim3((uint32_t)(nx * ny)),
                         dim3(256), 0, s, X, nq, Yc, cc, wp, (uint32_t)nx, cb,
                         bitmap, radius, counts, lims, cursors, out);
    else
      hipLaunchKernelGGL(k_hamming_range<false>, dim3((uint32_t)(nx * ny)),
                         dim3(256), 0, s, X, nq, Yc, cc, wp, (uint32_t)nx, cb,
                         bitmap, radius, counts, lims, cursors, out);
  }
}

void argmin_score(hipStream_t s, const float* scores, int64_t n, int32_t cols,
                  int32_t* out) {
  if (n) hipLaunchKernelGGL(k_argmin_score, dim3(ceil_div(n, 4)),
                            dim3(4 * WAVE), 0, s, scores, n, cols, out);
}

void bivf_scan(hipStream_t s, const uint32_t* units, int32_t n_units,
               const int64_t* csr_offsets, const int32_t* chunk_off,
               const int64_t* chunk_base, const uint32_t* twords,
               const uint32_t* queries, int32_t wp,
               const int32_t* inv_offsets, const int32_t* inv_q,
               const int32_t* inv_rank, const int64_t* qp_off,
               const int64_t* q_cand_base, int32_t nprobe,
               const uint32_t* bitmap, int32_t chunk_rows, uint64_t* cand) {
  if (!n_units) return;
  constexpr int QT = 8;  // 32 accumulators per thread; LDS = wp * 32 B
  hipLaunchKernelGGL(k_bivf_scan<QT>, dim3((uint32_t)n_units), dim3(256),
                     (size_t)wp * QT * 4, s, units, csr_offsets, chunk_off,
                     chunk_base, twords, queries, wp, inv_offsets, inv_q,
                     inv_rank, qp_off, q_cand_base, nprobe, bitmap,
                     chunk_rows, cand);
}

void bits_to_pm1(hipStream_t s, const uint32_t* x, int64_t n, int32_t d,
                 int32_t wp, float* out) {
  if (n) hipLaunchKernelGGL(k_bits_to_pm1, dim3(ceil_div(n * d, 256)),
                            dim3(256), 0, s, x, n, d, wp, out);
}

void binarise(hipStream_t s, const float* c, int64_t n, int32_t d, int32_t wp,
              uint32_t* out) {
  if (n) hipLaunchKernelGGL(k_binarise, dim3(ceil_div(n * wp, 256)), dim3(256),
                            0, s, c, n, d, wp, out);
}

}  // namespace dgk
