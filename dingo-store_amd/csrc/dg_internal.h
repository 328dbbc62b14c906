// dg_internal.h — internal state of the MI355X-native index library.
// Product path: no oracle code is linked or called here (oracle/ is test
// infrastructure only).  All compute runs on the GPU; there is no CPU
// fallback — entry points fail with DG_ENOGPU when no device is present.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dingo_gpu.h"
#include "dg_coarse_wave.h"
#include "dg_scan_split.h"

#define DG_HIP_CHECK(expr)                                              \
  do {                                                                  \
    hipError_t _e = (expr);                                             \
    if (_e != hipSuccess) {                                             \
      dg_set_error("HIP error %s at %s:%d: %s", hipGetErrorName(_e),    \
                   __FILE__, __LINE__, hipGetErrorString(_e));          \
      return DG_EINTERNAL;                                              \
    }                                                                   \
  } while (0)

#define DG_ROCBLAS_CHECK(expr)                                          \
  do {                                                                  \
    rocblas_status _s = (expr);                                         \
    if (_s != rocblas_status_success) {                                 \
      dg_set_error("rocBLAS error %d at %s:%d", (int)_s, __FILE__,      \
                   __LINE__);                                           \
      return DG_EINTERNAL;                                              \
    }                                                                   \
  } while (0)

void dg_set_error(const char* fmt, ...);

// Internal ingestion used by the faiss-file loader (faiss_io.cpp): uploads
// rows with their FILE-stored coarse assignment (recomputing on GPU could
// flip fp ties vs the CPU faiss reading the same file) and without
// re-normalizing (file data is already in stored form).  x for Flat/IVF,
// codes for PQ.  Takes the write lock itself.
dg_status dg_ingest_rows(dg_index* ix, int64_t n, const int64_t* ids,
                         const float* x, const uint8_t* codes,
                         const int32_t* assign);

// The same for the binary kinds: rows of d/8 packed bytes (no word padding),
// assign = null for Flat.
dg_status dg_ingest_bits(dg_index* ix, int64_t n, const int64_t* ids,
                         const uint8_t* bits, const int32_t* assign);

// One flush of the search batcher (dg_batch.cpp): dg_search_device /
// dg_search_binary_device under the same locks, except that only a flush of
// one query may capture the small-batch hipGraph.  A flush of 2..4 queries
// replays a graph that matches and otherwise runs the kernels, so changing
// flush sizes never recapture (search batching).
dg_status dg_search_device_flush(dg_index* ix, int64_t nq, const void* d_x,
                                 int32_t k, int32_t nprobe,
                                 const dg_filter* filter, float* d_out_dist,
                                 int64_t* d_out_ids, bool binary_entry);
// dg_index_destroy: drains and frees the index's batcher, if it has one
struct dg_batcher;
void dg_batcher_destroy(dg_batcher* b);

// The sharded index (dg_shard.cpp) checks presence before it touches a shard:
// true iff id is a live row of ix.  Takes the read lock itself.
bool dg_contains_id(dg_index* ix, int64_t id);

// Device-side filter descriptor (POD copied into kernel args).
struct dg_dev_filter {
  int32_t kind;    // dg_filter_kind
  int32_t negate;
  int64_t min_id, max_id;
  const int64_t* ids;       // device pointer (uploaded), ascending
  int64_t n_ids;
  const uint64_t* bitmap;   // device pointer
  int64_t bitmap_base, bitmap_nbits;
};

// A growable device buffer.
struct dg_dbuf {
  void* p = nullptr;
  size_t bytes = 0, cap = 0;
};

// kind helpers: the binary kinds share the Flat / IVF-Flat machinery
static inline bool dg_kind_is_binary(int32_t kind) {
  return kind == DG_INDEX_BINARY_FLAT || kind == DG_INDEX_BINARY_IVF_FLAT;
}
static inline bool dg_kind_is_flat(int32_t kind) {
  return kind == DG_INDEX_FLAT || kind == DG_INDEX_BINARY_FLAT;
}

// IVF-PQ geometry: codewords per subspace and bytes of one packed code row
// (nbits = 8: one byte per sub-quantizer; nbits = 4: faiss's generic PQ
// packing, sub-quantizer 2j in the low nibble of byte j, 2j+1 in the high)
static inline int32_t dg_pq_ksub(const dg_index_desc& d) {
  return 1 << d.pq_nbits;
}
static inline int32_t dg_pq_code_size(const dg_index_desc& d) {
  return d.pq_m * d.pq_nbits / 8;
}

// DG_INDEX_HNSW keeps its graph, its host rows and its device mirror in a
// state of its own (dg_hnsw.cpp); the Flat / IVF members of dg_index below
// stay unused for that kind, except the stream, the events, the counts and
// the locks.
struct dg_hnsw_state;
static inline bool dg_kind_is_hnsw(int32_t kind) {
  return kind == DG_INDEX_HNSW;
}

struct dg_stage_times {
  double coarse_ms = 0, scan_ms = 0, select_ms = 0, total_ms = 0;
  // cumulative since last reset (for bench averaging)
  double acc_scan_ms = 0;
  int64_t acc_scan_launches = 0;
  int64_t last_scan_bytes_alg = 0;
  int64_t last_nq = 0;
  // binary Flat range search: the scan is two kernel passes with host work
  // between them, timed as ev[6..7] + ev[8..9] instead of ev[2..3]
  bool scan_split = false;
};

struct dg_index {
  // INTERNAL dimension convention: desc.d is PADDED to a multiple of 4
  // (zero-filled pad columns — dots and norms are unaffected); d_user is
  // the caller's dimension, the row stride of every pointer crossing the
  // ABI.  Boundary copies are 2D (pitched) when d_user != desc.d.
  dg_index_desc desc;
  int32_t d_user = 0;
  // Binary (Hamming) kinds: desc.d == d_user == dimension in BITS; rows,
  // queries and centroids are held as b_wp = ceil(d/32) zero-padded u32
  // words (DESIGN.md §Binary indexes).  The arrival store is d_codes
  // ([ntotal x b_wp] words), the grouped row-major rows d_csr_codes (Flat
  // only), the word-major chunks d_csr_t, the centroids d_centroids.
  bool is_bin = false;
  int32_t b_wp = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  rocblas_handle blas = nullptr;

  // ---- store (arrival order; the base of truth) ----
  dg_dbuf d_vectors;   // [ntotal x d] f32 (normalized already for cosine);
                       // halves when storage == DG_STORAGE_F16
  // Row storage (dg_set_storage; IVF-Flat only).  It is not part of
  // dg_index_desc, which dg_save writes raw.  With DG_STORAGE_F16 the
  // arrival store and the chunks d_csr_t hold IEEE halves; centroids,
  // assignment, queries and d_csr_vnorms (norms of the decoded rows) stay
  // f32.
  int32_t storage = DG_STORAGE_F32;
  size_t elem_bytes() const {
    return storage == DG_STORAGE_F16 ? 2 : storage == DG_STORAGE_SQ8 ? 1 : 4;
  }
  // DG_STORAGE_SQ8: per-dimension ranges of the codec (dg_sq8_core.h).  The
  // host copies are what dg_get_sq_ranges and dg_save return; d_sq holds
  // [vmin d][vdiff d][step d] floats at the padded d (pad dims are 0).  An
  // SQ8 index is trained when it has centroids (trained) and ranges.
  bool sq_has_ranges = false;
  std::vector<float> h_sq_vmin, h_sq_vdiff;  // [d_user]
  dg_dbuf d_sq;
  dg_dbuf ws_sq8q;  // per batch: q' [nq x d] then cq [nq] (k_sq8_fold_query)
  bool is_ready() const {
    return trained && (storage != DG_STORAGE_SQ8 || sq_has_ranges);
  }
  bool last_scan_sq8 = false;  // the last search_core scan was k_ivf_scan_sq8
  bool last_scan_f16 = false;  // the last search_core scan was k_ivf_scan_f16
  dg_dbuf d_ids;       // [ntotal] i64
  dg_dbuf d_assign;    // [ntotal] i32 (IVF only; coarse list per vector)
  int64_t ntotal = 0;
  int64_t n_deleted = 0;

  // ---- IVF structure ----
  bool trained = false;
  dg_dbuf d_centroids;      // [nlist x d]
  dg_dbuf d_cnorms;         // [nlist] f32  (L2 coarse via norms trick)
  // finalized CSR (built lazily from arrival store on first search)
  bool csr_valid = false;
  dg_dbuf d_csr_offsets;    // [nlist+1] i64
  dg_dbuf d_csr_vectors;    // FLAT: [ntotal x d] row-major (rocBLAS dots)
  dg_dbuf d_csr_ids;        // [ntotal] i64 (-2 = deleted tombstone)
  dg_dbuf d_csr_vnorms;     // [ntotal] f32 norms in CSR row order
  std::vector<int64_t> h_csr_offsets;  // host copy for planning
  std::vector<int64_t> h_len_prefix_desc;  // prefix of list lens sorted
                                           // desc: candidate upper bounds
  int64_t* h_pinned = nullptr;  // pinned: async alg-bytes readback
  // IVF: column-major 1024-row chunks ([d][nrows_pad] per chunk) — the
  // layout the v2 scan kernel reads
  dg_dbuf d_csr_t;          // transposed chunk data
  dg_dbuf d_chunk_meta;     // chunk_off i32[nlist+1] + chunk_base i64[nchunks]
                            // + all-chunks unit array u32[2*nchunks]
  int32_t total_chunks = 0;
  static constexpr int32_t kChunkRows = 1024;
  // IVF-Flat top-k: the scan keeps each wave's k smallest candidates when
  // k <= kScanFuseMaxK (one result lane per rank, so at most 64); larger k
  // stores every candidate (DESIGN.md §Kernels has the measurement)
  static constexpr int32_t kScanFuseMaxK = 64;
  // grid.y of the pair scan: a list's tile pairs are strided over it
  // (DESIGN.md §Pair scan has the measurement)
  static constexpr int32_t kScanPairPY = 2;
  int32_t cpl_max = 0;      // 1024-row chunks of the longest list

  // Flat uses d_csr_* with a single implicit list (nlist=1) so scan/select
  // machinery is shared.

  // ---- IVF-PQ state ----
  bool pq_trained = false;
  // ksub = dg_pq_ksub (256 or 16), code_size = dg_pq_code_size (M or M/2)
  dg_dbuf d_codebooks;      // [M][ksub][dsub] f32
  dg_dbuf d_codes;          // arrival [ntotal x code_size] u8 (raw vectors
                            // are NOT kept for PQ; d_vectors stays empty)
  dg_dbuf d_csr_codes;      // grouped [ntotal x code_size] u8
  dg_dbuf d_S;              // [nlist][M][ksub] f16 ||c_m + cb||^2
  dg_dbuf d_cb_norms;       // [M][ksub] f32 codebook entry norms (encode)
  dg_dbuf ws_T;             // per-batch [nq][M][ksub] f16 q_sub . cb
  dg_dbuf ws_Tf32;          // f32 GEMM output before f16 convert

  // optional list ownership mask (multi-GPU list sharding)
  dg_dbuf d_list_mask;      // [nlist] u8, empty = all owned
  bool has_mask = false;

  // DG_INDEX_HNSW: everything but the members named at dg_hnsw_state above
  dg_hnsw_state* hnsw = nullptr;

  // id -> present (host, duplicate detection / remove)
  std::unordered_map<int64_t, int32_t> id_count;

  // workspaces (grown on demand, reused across searches)
  dg_dbuf ws_queries, ws_qnorms, ws_dots, ws_probes, ws_inv, ws_cand,
      ws_units, ws_small, ws_topk;
  // exclusive-scan block-sum scratch (1024 i64).  Per-index so concurrent
  // searches of DIFFERENT indexes (multi-region deployment) cannot race on
  // a process-wide static, and the buffer lives on the index's device
  // (ADVICE r01 high).  Serialized within an index by search_mu / rw-write.
  dg_dbuf ws_scan;
  // segmented-select slab (wide-k coarse top-nprobe merge)
  dg_dbuf ws_seg;
  // per-row pass bitmap (filters/tombstones) — index-owned so captured
  // graphs may reference it (see search_core)
  dg_dbuf ws_bm;
  // per-wave top-k slots of the fused IVF-Flat scan (replaces ws_cand there)
  dg_dbuf ws_partial;
  bool last_scan_fused = false;  // path of the last search_core IVF scan
  bool last_scan_mfma = false;   // ... and whether it was k_ivf_scan_mfma
  bool last_scan_pair = false;   // ... and whether k_ivf_scan_mfma2 ran too
  dg_dbuf ws_qimage;             // its operand image of the queries
  bool last_coarse_wave = false;  // the last IVF search ran k_coarse_select
  const int32_t* last_probes = nullptr;  // its probes array (in ws_probes)
  int64_t last_probes_n = 0;             // ... and its nq * np entries

  // timing
  hipEvent_t ev[12] = {};
  dg_stage_times times;
  bool events_ready = false;

  // ---- small-batch hipGraph cache (nq=1 latency path; the reference's
  // thread pool issues nq=1 per Search call, vector_index.cc:53-54) ----
  // Captured over search_core with fixed staging in/out buffers; replayed
  // when (nq, k, nprobe) match and the index generation is unchanged.
  hipGraphExec_t graph_exec = nullptr;
  int32_t graph_nq = 0, graph_k = 0, graph_np = 0;
  bool graph_fused = false;  // DG_SCAN_FUSED state the graph was captured in
  bool graph_mfma = false;   // DG_SCAN_MFMA state, likewise
  int32_t graph_pair = 0;    // DG_SCAN_PAIR state, likewise
  bool graph_cwave = false;  // DG_COARSE_WAVE state, likewise
  uint64_t graph_gen = 0;   // generation the graph was captured at
  uint64_t index_gen = 1;   // bumped on finalize/mutation/buffer growth
  dg_dbuf ws_gq, ws_gout;   // fixed staging: queries in, dist+ids out
  bool capturing = false;   // search_core: skip event records in capture

  // dg_batching_enable creates it; it lives until dg_index_destroy
  std::atomic<dg_batcher*> batcher{nullptr};

  std::shared_mutex rw;  // search shared; mutation exclusive
  // Concurrent dg_search calls are SAFE but serialized per index: searches
  // share the workspace buffers and the HIP stream, so execution holds this
  // mutex (the reference serializes device work on one stream anyway;
  // intra-index parallelism comes from batching, SURVEY.md §8b threading).
  std::mutex search_mu;
  // Stream capture is a property of the stream, not of the capturing thread:
  // a copy or a synchronize another thread issues on ix->stream while the
  // small-batch graph is being captured would be recorded into the graph
  // (with that caller's host pointer) or fail.  The capture holds this
  // exclusively; the host-pointer entry points and the batcher's flush hold
  // it shared around the stream calls they make outside search_mu.  Never
  // held while waiting for search_mu or rw.
  std::shared_mutex capture_mu;
};

// ---- DG_INDEX_HNSW (dg_hnsw.cpp): what the generic entry points of
// dg_abi.cpp, dg_batch.cpp and dg_shard.cpp dispatch to ----
dg_status dg_hnsw_create_state(dg_index* ix);
void dg_hnsw_destroy_state(dg_index* ix);
dg_status dg_hnsw_add(dg_index* ix, int64_t n, const int64_t* ids,
                      const float* x, bool x_on_device, bool upsert);
dg_status dg_hnsw_remove(dg_index* ix, int64_t n, const int64_t* ids);
dg_status dg_hnsw_reconstruct(dg_index* ix, int64_t n, const int64_t* ids,
                              float* out);
dg_status dg_hnsw_stats(dg_index* ix, dg_stats_out* out);
bool dg_hnsw_contains_id(dg_index* ix, int64_t id);
// the host form of the search (dg_abi.cpp: it owns the per-thread staging),
// and what it calls after its synchronise: DG_EINTERNAL if a wave of the
// last search raised the kernel's flag
dg_status dg_hnsw_search_host(dg_index* ix, int64_t nq, const float* x,
                              int32_t k, int32_t ef_search,
                              const dg_filter* filter, float* out_dist,
                              int64_t* out_ids);
dg_status dg_hnsw_after_sync(dg_index* ix);
// ef_search 0..1024 (else DG_EINVAL), k <= 1024 (else DG_ENOT_SUPPORT): the
// host form asks before it stages anything
dg_status dg_hnsw_check_search_args(int32_t k, int32_t ef_search);

// ---- kernel launchers (kernels.hip.cpp; authoritative signatures) ----
namespace dgk {
// ---- HNSW (hnsw.hip.cpp) ----
// the device mirror of a dg_hnsw::Graph (dg_hnsw_core.h), passed by value
struct hnsw_graph {
  const float* rows;        // [n][d] f32, d padded to a multiple of 4
  const int32_t* cnt0;      // level 0: count[n], links[n][maxM0]
  const uint32_t* links0;
  const int32_t* levels;    // [n]
  const int64_t* up_off;    // [n + 1] first list of node i at levels >= 1
  const int32_t* up_cnt;    // per list
  const uint32_t* up_links; // per list, maxM slots
  const uint32_t* pass;     // bit per node: not deleted and passes the filter
  const int64_t* ids;       // external id per node
  int64_t n, entry;
  int32_t d, maxM, maxM0, max_level, metric;
};
// dynamic LDS of one k_hnsw_search block (one wave): the query, C and W of
// ef' packed entries each and the neighbour staging
size_t hnsw_search_lds(int32_t d, int32_t efp);
// one wave per query; queries [nq][d_user]; visited = nq * vwords zeroed
// words (vwords = ceil(n / 32)); counters[2] += (expansions, dist_evals);
// *flag |= 1 if a wave met a bad link or the iteration cap.  Needs n > 0,
// 1 <= k <= efp <= 1024.
void hnsw_search(hipStream_t s, const hnsw_graph& g, const float* queries,
                 int64_t nq, int32_t d_user, int32_t k, int32_t efp,
                 uint32_t* visited, int64_t vwords, float* out_dist,
                 int64_t* out_ids, unsigned long long* counters,
                 int32_t* flag);
void probe_unpack(hipStream_t s, const uint64_t* topk, int64_t nq,
                  int32_t nprobe, const uint8_t* mask, int32_t* probes);
void probes_all(hipStream_t s, int64_t nq, int32_t nprobe,
                const uint8_t* mask, int32_t* probes);
void init_cursors(hipStream_t s, const int64_t* offsets, int32_t n,
                  int32_t* cursors);
// top-k per row over a dense scores matrix.  nseg > 1 splits columns into
// nseg segments (one block each, k results per segment at out_offset+seg*k;
// caller merges with select_u64).  ld = row stride of scores.
void select_dense(hipStream_t s, const float* scores, const float* cnorms,
                  int64_t rows, int64_t cols, int64_t ld, int32_t nseg,
                  int32_t k, int mode, const uint32_t* bitmap,
                  int64_t col_base, uint64_t* out, int64_t out_stride,
                  int64_t out_offset);
int select_dense_threads(int32_t k);
void select_u64(hipStream_t s, const uint64_t* cand, const int64_t* base,
                const int64_t* total, int64_t nq, int32_t k, uint64_t* out,
                int64_t out_stride);
void gather_rows_by_index(hipStream_t s, const float* src, const int64_t* idx,
                          int64_t n, int32_t d, float* dst);
void fill_base_total(hipStream_t s, int64_t nq, int64_t len, int64_t* base,
                     int64_t* total);
// select_u64 over uniform segments: query q's candidates are the len entries
// from cand + q * len (no base / total arrays)
void select_u64_uniform(hipStream_t s, const uint64_t* cand, int64_t len,
                        int64_t nq, int32_t k, uint64_t* out,
                        int64_t out_stride);
// coarse top-np of dots[nq][nlist] straight to probes[nq][np] (ascending
// packed key, masked lists -1), counting every probe >= 0 into counts, which
// the caller has zeroed.  Needs dg_coarse_wave_applies(np, nlist).
void coarse_select(hipStream_t s, const float* dots, const float* cnorms,
                   int64_t nq, int32_t nlist, int32_t np, int mode,
                   const uint8_t* mask, int32_t* probes, int32_t* counts);
// exclusive scan of counts[nlist] to off64 / off32 (nlist + 1 entries) and
// cursors (nlist) in one block.  Needs dg_inv_offsets_applies(nlist).
void inv_offsets(hipStream_t s, const int32_t* counts, int32_t nlist,
                 int64_t* off64, int32_t* off32, int32_t* cursors);
void tombstone(hipStream_t s, const int64_t* pos, int64_t n, int64_t* ids);
// binary (Hamming) indexes: packed u32 words, wp words per row
// out[nq x cols] (row stride ld) = popcount(X[q] ^ Y[c]) as exact f32
void hamming_dists(hipStream_t s, const uint32_t* X, int64_t nq,
                   const uint32_t* Y, int64_t cols, int32_t wp, float* out,
                   int64_t ld);
// Binary Flat range search, fused distance + radius test (no dists matrix).
// compact = false adds each query's hit count to counts[nq] (lims, cursors,
// out unused); compact = true appends pack(distance, row) for every hit at
// out[lims[q] + ...] through the zeroed cursors[nq] (counts unused).  A hit
// is a row whose bitmap bit is set (null bitmap: all) with distance < radius.
// The columns are covered by as many launches as max_blocks requires.
void hamming_range(hipStream_t s, bool compact, const uint32_t* X, int64_t nq,
                   const uint32_t* Y, int64_t cols, int32_t wp,
                   const uint32_t* bitmap, int32_t radius, int64_t* counts,
                   const int64_t* lims, int64_t* cursors, uint64_t* out,
                   int64_t max_blocks /* per launch, <= 2^30 */);
// per-row argmin of a dense score matrix, ties toward the smaller column
void argmin_score(hipStream_t s, const float* scores, int64_t n, int32_t cols,
                  int32_t* out);
void transpose_chunks_u32(hipStream_t s, const uint32_t* units,
                          int32_t n_units, const int64_t* csr_offsets,
                          const int32_t* chunk_off, const int64_t* chunk_base,
                          const uint32_t* rowmajor, int32_t wp,
                          int32_t chunk_rows, uint32_t* twords);
// store-all candidate scan over word-major chunks (key = f32 distance)
void bivf_scan(hipStream_t s, const uint32_t* units, int32_t n_units,
               const int64_t* csr_offsets, const int32_t* chunk_off,
               const int64_t* chunk_base, const uint32_t* twords,
               const uint32_t* queries, int32_t wp,
               const int32_t* inv_offsets, const int32_t* inv_q,
               const int32_t* inv_rank, const int64_t* qp_off,
               const int64_t* q_cand_base, int32_t nprobe,
               const uint32_t* bitmap, int32_t chunk_rows, uint64_t* cand);
void bits_to_pm1(hipStream_t s, const uint32_t* x, int64_t n, int32_t d,
                 int32_t wp, float* out);
void binarise(hipStream_t s, const float* c, int64_t n, int32_t d, int32_t wp,
              uint32_t* out);
void row_norms(hipStream_t s, const float* x, int64_t n, int32_t d,
               float* out);
void normalize_rows(hipStream_t s, float* x, int64_t n, int32_t d);
void argmin_rows(hipStream_t s, const float* dots, const float* cnorms,
                 int64_t n, int32_t nlist, int metric, int32_t* out);
// build per-row pass bitmap from filter over ids[row] (also kills tombstones)
void build_pass_bitmap(hipStream_t s, const int64_t* ids, int64_t n,
                       const dg_dev_filter* f, uint32_t* bitmap);
// IVF probe machinery
void hist_probes(hipStream_t s, const int32_t* probes, int64_t nq,
                 int32_t nprobe, int32_t nlist, int32_t* counts);
void scatter_probes(hipStream_t s, const int32_t* probes, int64_t nq,
                    int32_t nprobe, const int32_t* inv_offsets,
                    int32_t* cursors, int32_t* inv_q, int32_t* inv_rank);
void cand_offsets(hipStream_t s, const int32_t* probes, int64_t nq,
                  int32_t nprobe, const int64_t* csr_offsets,
                  int64_t* qp_off /* nq*nprobe, offset within query */,
                  int64_t* q_total /* nq */);
void fill_unit_counts(hipStream_t s, const int32_t* inv_counts, int32_t nlist,
                      const int64_t* csr_offsets, int32_t chunk_rows,
                      int32_t* unit_counts);
void alg_bytes(hipStream_t s, const int32_t* inv_counts,
               const int64_t* csr_offsets, int32_t nlist, int64_t row_bytes,
               int64_t* out /* device scalar, zeroed by caller */);
void fill_units(hipStream_t s, const int32_t* unit_offsets,
                const int32_t* inv_counts, int32_t nlist,
                const int64_t* csr_offsets, int32_t chunk_rows,
                uint32_t* units /* 2 x u32 per unit: list, chunk */,
                int32_t total_units);
void ivf_scan_col(hipStream_t s, const uint32_t* units, int32_t n_units,
                  const int64_t* csr_offsets, const int32_t* chunk_off,
                  const int64_t* chunk_base, const float* tvec,
                  const float* vnorms, const float* queries, int32_t d,
                  const int32_t* inv_offsets, const int32_t* inv_q,
                  const int32_t* inv_rank, const int64_t* qp_off,
                  const int64_t* q_cand_base, int32_t nprobe, int metric,
                  const uint32_t* bitmap, int32_t chunk_rows, uint64_t* cand,
                  int32_t mean_probes);
// IVF-Flat top-k scan with the per-wave selection fused in: writes the k
// (<= dg_index::kScanFuseMaxK) smallest candidates of each wave to
// partial[nq][nprobe][cpl_max][chunk_rows/256][k]; the caller presets
// partial to 0xff bytes (empty) and merges it with select_u64.  mfma picks
// k_ivf_scan_mfma (f32 MFMA dots) over k_ivf_scan_pipe (VALU dots); both
// fill the slots with the same bits.  With mfma, a non-null qimage
// (dg_scan_qimage_bytes(nq, d) bytes of workspace) and
// dg_scan_pair_applies(d, nq), lists probed by 17+ queries are scanned two
// query tiles per pass by k_ivf_scan_mfma2 on a (units, pair_py) grid.
void ivf_scan_topk(hipStream_t s, const uint32_t* units, int32_t n_units,
                   const int64_t* csr_offsets, const int32_t* chunk_off,
                   const int64_t* chunk_base, const float* tvec,
                   const float* vnorms, const float* queries, int32_t d,
                   const int32_t* inv_offsets, const int32_t* inv_q,
                   const int32_t* inv_rank, int32_t nprobe, int metric,
                   const uint32_t* bitmap, int32_t chunk_rows, int32_t k,
                   int32_t cpl_max, uint64_t* partial, bool mfma,
                   int64_t nq, float* qimage, int32_t pair_py);
void transpose_chunks(hipStream_t s, const uint32_t* units, int32_t n_units,
                      const int64_t* csr_offsets, const int32_t* chunk_off,
                      const int64_t* chunk_base, const float* rowmajor,
                      int32_t d, int32_t chunk_rows, float* tvec);
// ---- f16 row storage (DG_STORAGE_F16, IVF-Flat) ----
// out = round-to-nearest-even half of in; *overflow |= 1 if a component is
// NaN or exceeds the largest finite half
void f32_to_f16_check(hipStream_t s, const float* in, int64_t n, __half* out,
                      int32_t* overflow);
// squared norms of the decoded rows
void row_norms_f16(hipStream_t s, const __half* x, int64_t n, int32_t d,
                   float* out);
// dst[i] = decoded row idx[i] of src (d halves per row, d floats out)
void gather_rows_by_index_f16(hipStream_t s, const __half* src,
                              const int64_t* idx, int64_t n, int32_t d,
                              float* dst);
// row-major halves -> the chunk layout k_ivf_scan_f16 reads (kernels.hip.cpp
// documents it); chunk_base counts halves, a chunk is ceil(d/8)*8 x
// ceil(nrows/4)*4 of them
void transpose_chunks_f16(hipStream_t s, const uint32_t* units,
                          int32_t n_units, const int64_t* csr_offsets,
                          const int32_t* chunk_off, const int64_t* chunk_base,
                          const __half* rowmajor, int32_t d,
                          int32_t chunk_rows, __half* tvec);
// the IVF-Flat scan over f16 chunks, one dot-product body for both candidate
// flows: fused writes the per-wave top-k slots of ivf_scan_topk to out
// (qp_off / q_cand_base unused), otherwise every candidate goes to out in
// the layout of ivf_scan_col
void ivf_scan_f16(hipStream_t s, const uint32_t* units, int32_t n_units,
                  const int64_t* csr_offsets, const int32_t* chunk_off,
                  const int64_t* chunk_base, const __half* tvec,
                  const float* vnorms, const float* queries, int32_t d,
                  const int32_t* inv_offsets, const int32_t* inv_q,
                  const int32_t* inv_rank, const int64_t* qp_off,
                  const int64_t* q_cand_base, int32_t nprobe, int metric,
                  const uint32_t* bitmap, int32_t chunk_rows, bool fused,
                  int32_t k, int32_t cpl_max, uint64_t* out,
                  int32_t py /* grid.y: a list's tiles are strided over it */);
// ---- SQ8 row storage (DG_STORAGE_SQ8, IVF-Flat; dg_sq8_core.h) ----
// out = code of in ([n / d x d] f32 staging); *bad |= 1 on NaN or inf
void sq8_encode_check(hipStream_t s, const float* in, int64_t n, int32_t d,
                      const float* vmin, const float* vdiff, uint8_t* out,
                      int32_t* bad);
// squared norms of the decoded rows
void row_norms_sq8(hipStream_t s, const uint8_t* x, int64_t n, int32_t d,
                   const float* vmin, const float* vdiff, float* out);
// dst[i] = decoded row idx[i] of src (d bytes per row, d floats out)
void gather_rows_by_index_sq8(hipStream_t s, const uint8_t* src,
                              const int64_t* idx, int64_t n, int32_t d,
                              const float* vmin, const float* vdiff,
                              float* dst);
// qp = q * step, cq[i] = sum_j q_ij * (vmin_j + step_j / 2) (f64, rounded
// once): the affine decode folded into the query, once per batch
void sq8_fold_query(hipStream_t s, const float* q, int64_t nq, int32_t d,
                    const float* vmin, const float* step, float* qp,
                    float* cq);
// vmin = per-dimension min, vdiff = max - min (f32) of x [n x d]
void sq8_col_minmax(hipStream_t s, const float* x, int64_t n, int32_t d,
                    float* vmin, float* vdiff);
// row-major codes -> the chunk layout of dg_sq8_core.h; chunk_base counts
// bytes, a chunk is ceil(d/16)*16 x ceil(nrows/4)*4 of them
void transpose_chunks_sq8(hipStream_t s, const uint32_t* units,
                          int32_t n_units, const int64_t* csr_offsets,
                          const int32_t* chunk_off, const int64_t* chunk_base,
                          const uint8_t* rowmajor, int32_t d,
                          int32_t chunk_rows, uint8_t* tvec);
// ivf_scan_f16 over SQ8 chunks; qprime / cq come from sq8_fold_query
void ivf_scan_sq8(hipStream_t s, const uint32_t* units, int32_t n_units,
                  const int64_t* csr_offsets, const int32_t* chunk_off,
                  const int64_t* chunk_base, const uint8_t* tvec,
                  const float* vnorms, const float* qprime, const float* cq,
                  int32_t d, const int32_t* inv_offsets, const int32_t* inv_q,
                  const int32_t* inv_rank, const int64_t* qp_off,
                  const int64_t* q_cand_base, int32_t nprobe, int metric,
                  const uint32_t* bitmap, int32_t chunk_rows, bool fused,
                  int32_t k, int32_t cpl_max, uint64_t* out, int32_t py);
// range search
void range_emit(hipStream_t s, const uint64_t* packed, const int64_t* lims,
                const int64_t* ids_lookup, const float* qnorms, int64_t nq,
                int metric, int add_qnorm, float* out_dist,
                int64_t* out_ids);
// Candidate variants: thr != nullptr (binary kinds) admits packed keys below
// thr[q]; thr == nullptr (float kinds) admits on the number range_emit
// writes, max(0, key + qnorms[q]) < radius for metric L2 and -key > radius
// for IP / COSINE (qnorms is read for L2 only).  The dense variants are the
// float form over a dots chunk, mode 1 (L2) or 2 (IP / COSINE).
void count_below(hipStream_t s, const uint64_t* cand, const int64_t* base,
                 const int64_t* total, const uint64_t* thr, int metric,
                 const float* qnorms, float radius, int64_t nq,
                 int64_t* counts);
void compact_below(hipStream_t s, const uint64_t* cand, const int64_t* base,
                   const int64_t* total, const uint64_t* thr, int metric,
                   const float* qnorms, float radius, const int64_t* out_off,
                   int64_t nq, int64_t* cursors, uint64_t* out);
void count_below_dense(hipStream_t s, const float* scores,
                       const float* cnorms, int64_t rows, int64_t cols,
                       int mode, const uint32_t* bitmap, int64_t col_base,
                       const float* qnorms, float radius, int64_t* counts);
void compact_below_dense(hipStream_t s, const float* scores,
                         const float* cnorms, int64_t rows, int64_t cols,
                         int mode, const uint32_t* bitmap, int64_t col_base,
                         const float* qnorms, float radius,
                         const int64_t* out_off, int64_t* cursors,
                         uint64_t* out);
// IVF-PQ
void residual(hipStream_t s, const float* x, const int32_t* assign,
              const float* centroids, int64_t n, int32_t d, float* out);
// writes sub-quantizer m of every row (code_size bytes per row).  nbits = 4
// packs two per byte: even m stores the byte, odd m ORs its high nibble in,
// so the per-m launches must be ordered (one stream) and ascend in m
void set_code(hipStream_t s, const int32_t* amin, int64_t n, int32_t m,
              int32_t code_size, int32_t nbits, uint8_t* codes);
// M = bytes per row, a multiple of 4
void gather_codes(hipStream_t s, const uint8_t* src, const uint32_t* perm,
                  int64_t n, int32_t M, uint8_t* dst);
void build_S(hipStream_t s, const float* centroids, const float* codebooks,
             int32_t nlist, int32_t M, int32_t ksub, int32_t dsub, int32_t d,
             __half* S,
             int32_t* overflow);  // *overflow |= 1 if an entry exceeds f16
// rows of the default k_ivfpq_scan tile (RPV=4 x 64 lanes)
constexpr int32_t kPqTileRows = 256;
size_t max_launch_lds();  // dynamic LDS per launch, current device
size_t ivfpq_scan_lds(int32_t tile_rows, int32_t M);
// LDS of one k_ivfpq4_scan block (nbits = 4, 256-row tiles)
size_t ivfpq4_scan_lds(int32_t M);
void f32_to_f16(hipStream_t s, const float* in, int64_t n, __half* out);
// returns the launch status; no launch is issued if the tile's LDS does
// not fit the device.  nbits = 8: csr_codes rows of M bytes, S and T rows of
// 256 entries; nbits = 4: packed rows of M/2 bytes, 16-entry S and T rows
hipError_t ivfpq_scan(hipStream_t s, const uint32_t* units, int32_t n_units,
                      const int64_t* csr_offsets, const uint8_t* csr_codes,
                      const __half* S, const __half* T,
                      const float* coarse_dots, int32_t nlist, int32_t M,
                      const int32_t* inv_offsets, const int32_t* inv_q,
                      const int32_t* inv_rank, const int64_t* qp_off,
                      const int64_t* q_cand_base, int32_t nprobe, int metric,
                      const uint32_t* bitmap, int32_t chunk_rows,
                      uint64_t* cand, int32_t nbits);
// emit: resolve ids, apply metric convention
void emit_results(hipStream_t s, const uint64_t* topk,
                  const int64_t* ids_lookup, const float* qnorms, int64_t nq,
                  int32_t k, int metric, int add_qnorm, float* out_dist,
                  int64_t* out_ids);
// merge n_lists best-first lists per query into the k_out best under the
// order of dg_shard_core.h: dists / ids [n_lists][nq][k_in] ->
// out [nq][k_out], rank placement, one thread per input element.  The caller
// checks the limits (n_lists <= 32, k_in, k_out <= 2048, block count)
void merge_lists(hipStream_t s, const float* dists, const int64_t* ids,
                 int32_t n_lists, int64_t nq, int32_t k_in, int32_t k_out,
                 int metric, float* out_dist, int64_t* out_ids);
// k-means / finalize helpers
void dots_mfma(hipStream_t s, const float* X, int64_t M, const float* Y,
               int64_t N, int32_t K, float* C, int64_t ldc);
void hist_assign(hipStream_t s, const int32_t* assign, int64_t n,
                 int32_t nlist, int32_t* counts);
void identity_perm(hipStream_t s, int64_t n, uint32_t* perm);
void scatter_perm(hipStream_t s, const int32_t* assign, int64_t n,
                  const int64_t* offsets_i64, int32_t* cursors32,
                  uint32_t* perm /* dest slot for row i */);
void gather_rows(hipStream_t s, const float* src, const uint32_t* perm,
                 int64_t n, int32_t d, float* dst);
void gather_ids(hipStream_t s, const int64_t* src, const uint32_t* perm,
                int64_t n, int64_t* dst);
void cluster_means(hipStream_t s, const float* grouped, const int64_t* offsets,
                   int32_t nlist, int32_t d, float* centroids);
void iota_i32(hipStream_t s, int32_t* p, int64_t n, int32_t value);
// block_sums: caller-owned device scratch of >= 1024 i64 (dg_index::ws_scan)
void excl_scan_i32_to_i64(hipStream_t s, const int32_t* in, int32_t n,
                          int64_t* out /* n+1 */, int64_t* block_sums);
void excl_scan_i64(hipStream_t s, const int64_t* in, int64_t n,
                   int64_t* out /* n+1 */, int64_t* block_sums);
}  // namespace dgk
