/* dingo_gpu.h — C-ABI of the MI355X-native vector-index search path for
 * dingo-store's Index role.
 *
 * This is the drop-in boundary defined in SURVEY.md §8(b): the set of entry
 * points a replacement of the reference's VectorIndex plugin surface
 * (reference: src/vector/vector_index.h:56-279, concrete indexes
 * src/vector/vector_index_{flat,ivf_flat,raw_ivf_pq}.cc) must export.  The
 * C++ host mirror in dingo-store_amd/host/ re-declares the reference's
 * plugin virtuals (Search/RangeSearch/Add/Upsert/Delete/Train/Save/Load,
 * vector_index.h:148-229) on top of exactly these functions; a dingo-store
 * maintainer binds them from the Index role as shown in INTEGRATION.md.
 *
 * Conventions (mirroring the reference call sites):
 *  - Caller owns every in/out buffer except range-search results (dg_free).
 *  - No exceptions cross the ABI: int status + dg_last_error().
 *  - Distances are returned in faiss convention (L2: raw squared distance,
 *    IP/cosine: raw score, larger = better).  The observable dingo-store
 *    semantics — IP/cosine reported as 1.0f - score, L2 passed through —
 *    are applied by the C++ shim, restating
 *    src/vector/vector_index_utils.cc:612-655 (the flip at :634).
 *  - out_ids is padded with -1 where fewer than k results exist, like the
 *    labels pre-fill at src/vector/vector_index_flat.cc:218 and
 *    src/vector/vector_index_ivf_flat.cc:217.
 *  - Thread-safety: concurrent dg_search calls are safe but run one at a
 *    time per index (they share its stream and workspaces), so N threads
 *    with one query each get the throughput of one.  dg_search_batched
 *    merges such calls into device batches (see "search batching" below).
 *    dg_add / dg_remove / dg_train / dg_load are exclusive (host RW lock
 *    mirroring the reference's RWLock usage,
 *    src/vector/vector_index_ivf_flat.cc:109,225).
 */
#ifndef DINGO_GPU_H_
#define DINGO_GPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dg_status {
  DG_OK = 0,
  DG_EINVAL = 1,        /* pb::error::EILLEGAL_PARAMTETERS */
  DG_ENOT_TRAINED = 2,  /* pb::error::EVECTOR_NOT_TRAIN */
  DG_ENOT_SUPPORT = 3,  /* pb::error::EVECTOR_NOT_SUPPORT — triggers the
                           reader's brute-force fallback,
                           src/vector/vector_reader.cc:1828-1831 */
  DG_ENOMEM = 4,
  DG_EINTERNAL = 5,     /* pb::error::EINTERNAL */
  DG_EIO = 6,
  DG_ENOGPU = 7,        /* HIP device unavailable: the product path fails
                           loudly, it never falls back to CPU */
  DG_EID_DUPLICATED = 8,/* pb::error::EVECTOR_ID_DUPLICATED */
  DG_ENOT_FOUND = 9     /* pb::error::EVECTOR_INVALID (remove miss),
                           src/vector/vector_index_ivf_flat.cc:183 */
} dg_status;

typedef enum dg_index_kind {
  DG_INDEX_FLAT = 0,     /* VectorIndexFlat: faiss IndexFlatL2/IP + IDMap2,
                            src/vector/vector_index_flat.cc:81-98 */
  DG_INDEX_IVF_FLAT = 1, /* VectorIndexIvfFlat: faiss IndexIVFFlat,
                            src/vector/vector_index_ivf_flat.cc:805-823 */
  DG_INDEX_IVF_PQ = 2,   /* VectorIndexRawIvfPq: faiss IndexIVFPQ,
                            src/vector/vector_index_raw_ivf_pq.cc:551-570 */
  DG_INDEX_BINARY_FLAT = 3,     /* VectorIndexFlat<faiss::IndexBinary,
                                   IndexBinaryIDMap2>,
                                   src/vector/vector_index_flat.cc:71,99-102 */
  DG_INDEX_BINARY_IVF_FLAT = 4, /* VectorIndexIvfFlat<faiss::IndexBinary,
                                   IndexBinaryIVF>,
                                   src/vector/vector_index_ivf_flat.cc:62,75-80 */
  DG_INDEX_HNSW = 5      /* VectorIndexHnsw over hnswlib,
                            src/vector/vector_index_hnsw.cc ("HNSW" below) */
} dg_index_kind;

typedef enum dg_metric {
  DG_METRIC_L2 = 0,     /* METRIC_TYPE_L2 */
  DG_METRIC_IP = 1,     /* METRIC_TYPE_INNER_PRODUCT */
  DG_METRIC_COSINE = 2, /* METRIC_TYPE_COSINE = normalize + IP,
                           src/vector/vector_index_flat.cc:88-91 */
  DG_METRIC_HAMMING = 3 /* METRIC_TYPE_HAMMING: the binary kinds only (and
                           their only metric, vector_index_utils.cc:1094,1125) */
} dg_metric;

typedef struct dg_index dg_index; /* opaque */

typedef struct dg_index_desc {
  int32_t kind;      /* dg_index_kind */
  int32_t metric;    /* dg_metric */
  int32_t d;         /* dimension (binary kinds: in BITS, d % 8 == 0,
                        8 <= d <= 32768) */
  int32_t nlist;     /* IVF: ncentroids (reference default 2048,
                        src/vector/vector_index.h "kCreateIvfFlatParamNcentroids") */
  int32_t pq_m;      /* IVF-PQ: subquantizers (default 64) */
  int32_t pq_nbits;  /* IVF-PQ: bits per code, 4 or 8 (0 = default 8); every
                        other value is DG_ENOT_SUPPORT.  nbits = 4 needs
                        m % 8 == 0 besides d % 4 == 0 and d % m == 0 */
  int32_t device;    /* HIP device ordinal; -1 = current device */
  int64_t reserve;   /* capacity hint in vectors; 0 = grow on demand */
} dg_index_desc;

/* FilterFunctor forms, reference src/vector/vector_index.h:67-146:
 * RANGE      = RangeFilterFunctor   (min <= id < max), vector_index.h:77-80
 * SORTED_IDS = SortFilterFunctor    (binary search),   vector_index.h:109-146
 * BITMAP     = ConcreteFilterFunctor/IDSelectorBatch as a device bitmap
 * negate mirrors is_negation_ (vector_index.h:88-101). */
typedef enum dg_filter_kind {
  DG_FILTER_NONE = 0,
  DG_FILTER_RANGE = 1,
  DG_FILTER_SORTED_IDS = 2,
  DG_FILTER_BITMAP = 3
} dg_filter_kind;

typedef struct dg_filter {
  int32_t kind;            /* dg_filter_kind */
  int32_t negate;          /* 0 or 1 */
  int64_t min_id, max_id;  /* RANGE: [min_id, max_id) */
  const int64_t* ids;      /* SORTED_IDS: ascending, caller-owned */
  int64_t n_ids;
  const uint64_t* bitmap;  /* BITMAP: bit (id - bitmap_base) */
  int64_t bitmap_base;
  int64_t bitmap_nbits;
} dg_filter;

typedef struct dg_stats_out {
  int64_t ntotal;          /* GetCount, vector_index.h:150 */
  int32_t d;               /* GetDimension, vector_index.h:148 */
  int32_t metric;
  int32_t kind;
  int32_t nlist;
  int32_t is_trained;      /* IsTrained, vector_index.h:201 */
  int64_t device_bytes;    /* GetMemorySize, vector_index.h:152 */
  /* per-stage timings of the LAST dg_search, measured with hipEvents on the
   * index's own stream (GPU equivalent of the Tracker phase recorders,
   * src/common/tracker.h:131-190) */
  double last_coarse_ms;
  double last_scan_ms;     /* dominant kernel: inverted-list scan (IVF) or
                              flat distance+select (Flat) */
  double last_select_ms;
  double last_total_ms;
  int64_t last_nq;
  /* roofline accounting for the dominant kernel of the last search:
   * algorithmic bytes = one read of every probed list's vectors+ids
   * (grouped accounting, SURVEY.md §8d cfg C) */
  int64_t last_scan_bytes_algorithmic;
  double last_scan_gbps_algorithmic;
  /* tombstoned-but-uncompacted rows (GetDeletedCount, vector_index.h:151;
   * the reference's faiss path compacts on remove so it reports 0 — here
   * removes tombstone until the next finalize) */
  int64_t deleted_count;
} dg_stats_out;

/* ---- lifecycle ---- */
dg_status dg_index_create(dg_index** out, const dg_index_desc* desc);
void dg_index_destroy(dg_index* idx);

/* ---- train (IVF): k-means over n x d train vectors.
 * Semantics restated from src/vector/vector_index_ivf_flat.cc:644-712:
 * cosine => normalize train data first (:687-691); n < nlist => nlist
 * degrades to 1 (:676-680); already trained => OK no-op (:669-671).
 * faiss Clustering defaults (niter=25, max 256 points/centroid subsample,
 * seed 1234) restated in oracle/oracle.c and matched here. ---- */
dg_status dg_train(dg_index* idx, int64_t n, const float* x);
/* Inject/extract centroids so CPU oracle and GPU search identical structures
 * (BASELINE.md protocol).  set_centroids marks the index trained; on an
 * IVF-PQ index that has codebooks it rebuilds the ADC tables. */
dg_status dg_set_centroids(dg_index* idx, int32_t nlist, const float* centroids);
dg_status dg_get_centroids(dg_index* idx, float* out_centroids);
/* IVF-PQ codebook injection/extraction (m x ksub x (d/m) floats, ksub =
 * 2^nbits: 256 or 16), the PQ analog of dg_set_centroids for oracle-shared
 * parity (requires centroids set first; rebuilds the ADC tables).  nbits
 * must be the index's.
 * Code layout, on the device, in the own container and in "IwPQ" files:
 * nbits = 8 stores one byte per sub-quantizer (code_size = m); nbits = 4 is
 * faiss's generic PQ packing, sub-quantizer 2j in the low nibble of byte j
 * and 2j+1 in the high nibble (code_size = m/2). */
dg_status dg_set_codebooks(dg_index* idx, int32_t m, int32_t nbits,
                           const float* codebooks);
dg_status dg_get_codebooks(dg_index* idx, float* out_codebooks);
/* The IVF-PQ geometry of an index, as created or loaded (defaults resolved).
 * DG_EINVAL for any other kind. */
dg_status dg_pq_params(dg_index* idx, int32_t* m, int32_t* nbits);
/* IVF-PQ limits.  The scan keeps a 256-row code tile and one list's f16
 * table in LDS, 768 * m bytes per block: dg_index_create, dg_load and
 * dg_load_faiss return DG_ENOT_SUPPORT for m above dg_ivfpq_max_m(device)
 * (212 with the 160 KiB a launch may use on MI355X; 0 if there is no such
 * device).  The tables are f16: dg_set_codebooks, dg_train and the loaders
 * return DG_ENOT_SUPPORT if some ||centroid_sub + codeword||^2 exceeds
 * 65504.  |query_sub . codeword| has the same limit but is not checked
 * (IVF-PQ limits). */
int32_t dg_ivfpq_max_m(int32_t device);
/* The same limit per code width.  nbits = 8 is dg_ivfpq_max_m.  The nbits = 4
 * scan keeps the packed 256-row tile (odd dword row stride), the list's
 * 16-entry f16 tables and four per-wave f32 lookup tables in LDS, about
 * 416 * m + 1024 bytes per block: m <= 392 (a multiple of 8) on MI355X.
 * 0 for any other nbits or if there is no such device. */
int32_t dg_ivfpq_max_m_nbits(int32_t device, int32_t nbits);

/* ---- mutation (exclusive) ----
 * add restates faiss add_with_ids via VectorIndexIvfFlat::Add
 * (src/vector/vector_index_ivf_flat.cc:119-124): assign to nearest centroid,
 * append (vector, id) to that inverted list.  Duplicate ids in one call =>
 * DG_EID_DUPLICATED (src/vector/vector_index_utils.cc CheckVectorIdDuplicated).
 * upsert = remove-if-present + add (VectorIndexFlat::Upsert semantics). */
dg_status dg_add(dg_index* idx, int64_t n, const int64_t* ids, const float* x);
/* device-pointer add: d_x lives on the index's device (bench hot-path
 * ingestion; semantics identical to dg_add) */
dg_status dg_add_device(dg_index* idx, int64_t n, const int64_t* ids,
                        const float* d_x);
/* download the per-vector coarse assignment (arrival order, n = ntotal
 * including tombstones).  Lets the CPU-baseline leg rebuild the identical
 * IVF structure without re-running assignment on host. */
dg_status dg_export_assign(dg_index* idx, int32_t* out /* ntotal */);
dg_status dg_upsert(dg_index* idx, int64_t n, const int64_t* ids, const float* x);
/* remove: all ids must exist, else DG_ENOT_FOUND and nothing is removed
 * (src/vector/vector_index_ivf_flat.cc:177-186). */
dg_status dg_remove(dg_index* idx, int64_t n, const int64_t* ids);

/* ---- row storage (opt-in; dg_index_desc is unchanged) ----
 * DG_STORAGE_F16 keeps the rows of a DG_INDEX_IVF_FLAT index as IEEE halves:
 * the arrival store and the scanned chunks are half the size and a search
 * streams half the bytes.  It is accepted only while ntotal == 0 (trained or
 * not); on a non-empty index or a binary kind the call returns DG_EINVAL, on
 * FLAT and IVF_PQ DG_ENOT_SUPPORT.  DG_STORAGE_F32 on an empty float index
 * is always accepted.
 *   - Centroids, the coarse stage, the assignment and the queries stay f32.
 *     add / add_device / upsert assign each row from its f32 values (after
 *     the cosine normalisation), then store it rounded to nearest-even half.
 *   - A component that is NaN or exceeds 65504 in magnitude fails the whole
 *     call with DG_EINVAL before anything is appended; dg_upsert makes this
 *     check before it removes the existing ids, so a refused upsert leaves
 *     the index as it was.
 *   - An arrival store reserved at create (desc.reserve) is re-reserved for
 *     the same number of rows at the new component size.
 *   - A returned distance is the metric between the f32 query (never rounded
 *     to half) and the decoded stored row, summed in f32: what faiss QT_fp16
 *     computes.  For COSINE the stored row is half(f32 normalise(x)); it is
 *     used as stored and not renormalised, so its norm is 1 +- ~2^-12 and a
 *     cosine score can exceed 1 by that much.
 *   - top-k, range search, filters, tombstones, upsert, the list mask, the
 *     small-batch graph replay, dg_search_batched and dg_export_assign work
 *     as on an f32 index.  The pair scan is not ported: dg_last_scan_pair
 *     is 0.  dg_save writes a container of its own (dg_load reads both);
 *     dg_save_faiss returns DG_ENOT_SUPPORT, no CPU node could read it.
 *
 * DG_STORAGE_SQ8 keeps one byte per component: per-dimension 8-bit scalar
 * quantisation, the codec of faiss QT_8bit, in f32 with ranges (vmin, vdiff):
 *     encode  t = vdiff_j > 0 ? (x - vmin_j) / vdiff_j : 0, clamped to [0, 1],
 *             code = (uint8)(int)(255.0f * t)
 *     decode  vmin_j + ((code + 0.5f) / 255.0f) * vdiff_j
 * It is accepted, refused and left under exactly the rules of F16; leaving
 * SQ8 drops its ranges.  What differs from F16:
 *   - The index is trained when it has centroids AND ranges: dg_stats
 *     .is_trained, the blank search on an untrained index and DG_ENOT_TRAINED
 *     from add / upsert follow that.  dg_train on an SQ8 index without ranges
 *     computes them from all n training rows after the cosine normalisation:
 *     per-dimension min, and vdiff = max - min in f32 (faiss RS_minmax with
 *     argument 0); if centroids are already present it trains the ranges
 *     only.  dg_set_sq_ranges injects ranges instead.
 *   - A component outside its range saturates, as in faiss.  A NaN or
 *     infinite component fails the whole add / upsert with DG_EINVAL before
 *     anything moves (upsert checks before it removes).
 *   - A returned distance is the metric between the f32 query (never
 *     quantised) and the decoded row, accumulated in f32.  COSINE stores the
 *     code of the f32-normalised row and uses it as stored.
 *   - dg_reconstruct returns the decoded row.  dg_last_scan_pair is 0;
 *     dg_save writes the DGI2 container with the ranges, dg_save_faiss
 *     returns DG_ENOT_SUPPORT. */
typedef enum dg_storage {
  DG_STORAGE_F32 = 0,
  DG_STORAGE_F16 = 1,
  DG_STORAGE_SQ8 = 2
} dg_storage;
dg_status dg_set_storage(dg_index* idx, int32_t storage);
int32_t dg_get_storage(dg_index* idx); /* -1 for NULL */
/* Inject / read back the per-dimension ranges of an SQ8 index (the analogue
 * of dg_set_centroids for tests that share a structure with a reference).
 * Set: SQ8 storage and ntotal == 0, every value finite and vdiff[j] >= 0,
 * else DG_EINVAL.  Get: DG_ENOT_TRAINED while there are no ranges.  On an
 * index of other storage both return DG_EINVAL. */
dg_status dg_set_sq_ranges(dg_index* idx, const float* vmin /* d */,
                           const float* vdiff /* d */);
dg_status dg_get_sq_ranges(dg_index* idx, float* vmin /* d */,
                           float* vdiff /* d */);
/* The stored row of each id decoded to f32, out[n x d] at the caller's d
 * stride (for COSINE the normalised rows).  FLAT and IVF_FLAT, either
 * storage.  Every id must be live, else DG_ENOT_FOUND and out is untouched;
 * repeated ids are allowed.  IVF_PQ: DG_ENOT_SUPPORT; binary: DG_EINVAL.
 * Positions are looked up as dg_remove does (one id download per call). */
dg_status dg_reconstruct(dg_index* idx, int64_t n, const int64_t* ids,
                         float* out /* n x d */);

/* ---- search ----
 * Restates VectorIndexIvfFlat::Search (src/vector/vector_index_ivf_flat.cc:
 * 191-275): nprobe <= 0 => index default (80, clamped); nprobe clamped to
 * nlist (:234); untrained IVF => all ids -1, DG_OK (:223-227 "direct return
 * blank"); k <= 0 => DG_OK no-op (:201).  Flat ignores nprobe
 * (src/vector/vector_index_flat.cc:205-264).  Cosine queries are normalized
 * like ExtractVectorValue (src/vector/vector_index_utils.cc:564-609,480-491).
 * Host-pointer form: copies in/out and synchronizes. */
dg_status dg_search(dg_index* idx, int64_t nq, const float* x, int32_t k,
                    int32_t nprobe, const dg_filter* filter,
                    float* out_dist /* nq x k */,
                    int64_t* out_ids /* nq x k */);
/* Device-pointer form: x/out_dist/out_ids are device pointers on the index's
 * device; enqueues on the index stream, no synchronization (call dg_sync).
 * This is the resident-in-HBM hot path bench.py times. */
dg_status dg_search_device(dg_index* idx, int64_t nq, const float* d_x,
                           int32_t k, int32_t nprobe, const dg_filter* filter,
                           float* d_out_dist, int64_t* d_out_ids);
dg_status dg_sync(dg_index* idx);

/* ---- search batching: many threads, few queries each ----
 * The reference's search pool calls Search from 16 threads with one query
 * per call (src/vector/vector_index.cc:53-54,244-271).  Searches of one
 * index run one at a time, so that call shape pays the fixed cost of a
 * search per query.  With batching enabled on an index, dg_search_batched /
 * dg_search_binary_batched coalesce the calls that are waiting into one
 * device batch.  There is no dispatcher thread: the first caller of a batch
 * leads it and flushes as soon as the previous flush has left the device,
 * so a lone caller pays no added wait, and under load a batch holds
 * whatever arrived during the previous flush.
 *  - Not enabled (the default): the _batched calls are dg_search /
 *    dg_search_binary.
 *  - Enabled: a call blocks until its own rows are in its own buffers and
 *    returns what dg_search would for the same arguments.  Arguments are
 *    checked before the call joins a batch; argument errors, k <= 0 and
 *    k > 2048 are answered by dg_search itself and never reach a batch.
 *  - Calls merge if they resolve to the same nprobe (<= 0 => 80, clamped to
 *    nlist; ignored by Flat) and carry no filter, or RANGE filters with
 *    equal (min_id, max_id, negate).  A batch runs at the largest k of its
 *    members and each member receives the first k columns of its rows; that
 *    is exact, results being best-first under a total order.  A call is
 *    never split; a batch closes when the next call would overflow it.
 *  - A call with a SORTED_IDS or BITMAP filter, or with nq >= max_batch,
 *    runs directly as dg_search and is counted in `bypassed`.
 *  - Float indexes: which GEMM kernel serves the coarse stage depends on
 *    the number of rows in the device batch, so a result may differ from
 *    the nq = 1 call in the last bits of a distance (and in the order of
 *    rows that tie within them).  Binary results are identical.
 *  - A flush that fails returns its status to every member, each with the
 *    message in its own dg_last_error.
 *  - dg_add / dg_remove / dg_train / the loaders interleave between flushes
 *    as they do between searches.  dg_batching_disable waits for the open
 *    batches and makes later _batched calls pass through; dg_index_destroy
 *    disables first.  Range search is not batched.
 * max_batch 0 selects 64 (at most 1024); the staging for max_batch queries
 * (pinned host and device memory) is allocated at enable time and grows
 * only when a k above 128 arrives.  Enabling again drains, applies the new
 * options and zeroes the statistics. */
typedef struct dg_batch_opts {
  int32_t max_batch;    /* queries per device batch; 0 = default 64 */
  int32_t max_wait_us;  /* how long an open batch may wait for company after
                           the device is free; 0 (default) = never wait */
} dg_batch_opts;
typedef struct dg_batch_stats {
  int64_t calls;              /* valid _batched calls since enable */
  int64_t queries;            /* their query rows */
  int64_t flushes;            /* device batches run */
  int64_t max_flush_queries;  /* rows of the largest one */
  int64_t bypassed;           /* calls run directly (filter kind, nq) */
} dg_batch_stats;
dg_status dg_batching_enable(dg_index* idx, const dg_batch_opts* opts);
dg_status dg_batching_disable(dg_index* idx);
dg_status dg_batching_stats(dg_index* idx, dg_batch_stats* out);
dg_status dg_search_batched(dg_index* idx, int64_t nq, const float* x,
                            int32_t k, int32_t nprobe,
                            const dg_filter* filter,
                            float* out_dist /* nq x k */,
                            int64_t* out_ids /* nq x k */);
dg_status dg_search_binary_batched(dg_index* idx, int64_t nq,
                                   const uint8_t* x, int32_t k,
                                   int32_t nprobe, const dg_filter* filter,
                                   float* out_dist /* nq x k */,
                                   int64_t* out_ids /* nq x k */);

/* ---- range search ----
 * Restates VectorIndexIvfFlat::RangeSearch (vector_index_ivf_flat.cc:278-368):
 * radius in faiss convention (L2: dist < radius, IP/cos: score > radius; the
 * C++ shim applies the 1-r flip of :302-305); results best-first per query,
 * ties toward the smaller id.  A row is admitted on the very float that is
 * written to out_dists (L2: the squared distance clamped at 0), so every
 * returned element satisfies dist < radius (IP/cos: score > radius) as a
 * float32 comparison, and an L2 radius <= 0 returns nothing, the 0.0 of a
 * query equal to a stored row included (as the reference, which compares
 * the final value).  Rows whose exact distance is within float32 rounding
 * of the radius (Flat exact path) may fall on either side.
 * CSR out params: caller frees *out_ids / *out_dists with dg_free. ---- */
dg_status dg_range_search(dg_index* idx, int64_t nq, const float* x,
                          float radius, const dg_filter* filter,
                          int64_t* lims /* nq+1 */, int64_t** out_ids,
                          float** out_dists);
void dg_free(void* p);

/* ---- persistence (Save/Load, vector_index.h:168-170; snapshot files,
 * src/vector/vector_index_snapshot_manager.cc:583-599).  Own container
 * format v1 (documented in DESIGN.md) plus the faiss-compatible container
 * below. */
dg_status dg_save(dg_index* idx, const char* path);
dg_status dg_load(dg_index** out, const char* path, int32_t device);

/* ---- faiss-file-compatible persistence ----
 * The reference's snapshot/install cycle ships faiss::write_index files
 * (vector_index_snapshot_manager.cc:583-599; written at
 * vector_index_flat.cc:354, vector_index_ivf_flat.cc:398, loaded at
 * vector_index_flat.cc:368-462, vector_index_ivf_flat.cc:413-514).  These
 * functions emit/ingest the faiss 1.7.x container byte layout (the
 * reference's faiss fork is >= 1.7.3 — it uses faiss::SearchParameters,
 * vector_index_flat.cc:232):
 *   FLAT     -> IndexIDMap2{IndexFlatL2|IndexFlatIP}   ("IxM2"/"IxF2"/"IxFI")
 *   IVF_FLAT -> IndexIVFFlat                            ("IwFl")
 *   IVF_PQ   -> IndexIVFPQ (residual, nbits 8 or 4)     ("IwPQ")
 * Cosine indexes are written as IP over stored (normalized) vectors, like
 * the reference (vector_index_flat.cc:88-91); on load, pass
 * metric_override = DG_METRIC_COSINE to reconstruct a cosine index from an
 * IP-metric file (-1 keeps the file metric).  Tombstoned rows are dropped
 * at save.  Format notes and the byte-level layout are in DESIGN.md. */
dg_status dg_save_faiss(dg_index* idx, const char* path);
dg_status dg_load_faiss(dg_index** out, const char* path,
                        int32_t metric_override, int32_t device);

/* ---- binary (Hamming) indexes ----
 * DG_INDEX_BINARY_FLAT / DG_INDEX_BINARY_IVF_FLAT with DG_METRIC_HAMMING.
 * Rows, queries and centroids are bit vectors of desc.d bits, passed as
 * uint8 with a row stride of d/8 bytes (bit j = byte j/8, bit j%8).  The
 * calls restate the float ones above at the reference's binary call sites
 * (vector_index_flat.cc:151-153,224-239; vector_index_ivf_flat.cc:122-123,
 * 207-209,254-257,578-635): train unpacks to +-1 floats, runs the same
 * k-means and binarises the centroids with > 0; an IVF nlist <= 0 defaults
 * to 2048, nprobe <= 0 to 80.  out_dist holds the exact integer Hamming
 * distance as float32, passed through with no flip
 * (vector_index_utils.cc:640-650); ties on distance resolve toward the
 * smaller internal row, ties between lists toward the smaller list.
 * nq is limited to 261887 per call.  dg_remove, dg_export_assign,
 * dg_set_list_mask, dg_stats (d in bits), dg_sync, the write lock and
 * dg_index_destroy work unchanged.  The float entry points return
 * DG_EINVAL on a binary index and these return DG_EINVAL on a float one;
 * dg_range_search, dg_save and dg_save_faiss return DG_ENOT_SUPPORT on a
 * binary index (range search and the faiss container have the _binary
 * calls below; the own container v1 does not hold binary indexes). */
dg_status dg_train_binary(dg_index* idx, int64_t n, const uint8_t* x);
dg_status dg_set_centroids_binary(dg_index* idx, int32_t nlist,
                                  const uint8_t* centroids);
dg_status dg_get_centroids_binary(dg_index* idx, uint8_t* out_centroids);
dg_status dg_add_binary(dg_index* idx, int64_t n, const int64_t* ids,
                        const uint8_t* x);
dg_status dg_upsert_binary(dg_index* idx, int64_t n, const int64_t* ids,
                           const uint8_t* x);
dg_status dg_search_binary(dg_index* idx, int64_t nq, const uint8_t* x,
                           int32_t k, int32_t nprobe, const dg_filter* filter,
                           float* out_dist /* nq x k */,
                           int64_t* out_ids /* nq x k */);
/* device pointers, no synchronization, runs on the index stream */
dg_status dg_search_binary_device(dg_index* idx, int64_t nq,
                                  const uint8_t* d_x, int32_t k,
                                  int32_t nprobe, const dg_filter* filter,
                                  float* d_out_dist, int64_t* d_out_ids);

/* Binary range search (VectorIndexFlat/IvfFlat::RangeSearch over
 * faiss::IndexBinary, vector_index_flat.cc:304-308,
 * vector_index_ivf_flat.cc:290-292,342-352).  radius is an integer, as in
 * faiss::IndexBinary::range_search: a row is returned iff hamming(query,
 * row) < radius, so radius <= 0 returns nothing and radius > d every
 * admissible row (not removed, passing the filter, and for IVF in a probed
 * list: nprobe <= 0 => 80, clamped to nlist, list mask applied; Flat
 * ignores nprobe).  An untrained IVF index returns all-zero lims and DG_OK.
 * CSR results like dg_range_search: within a query ascending by (distance,
 * id), out_dists the exact integer distance as float32.  *out_ids and
 * *out_dists are set on every return (possibly to NULL) and may always be
 * handed to dg_free.  nq is limited to 261887 per call. */
dg_status dg_range_search_binary(dg_index* idx, int64_t nq, const uint8_t* x,
                                 int32_t radius, int32_t nprobe,
                                 const dg_filter* filter,
                                 int64_t* lims /* nq+1 */, int64_t** out_ids,
                                 float** out_dists);
/* Binary faiss containers (faiss::write_index_binary 1.7.x layout, the
 * snapshot files of the binary kinds: vector_index_flat.cc:355-356,380-381,
 * vector_index_ivf_flat.cc:399-400,424-425):
 *   BINARY_FLAT     -> IndexBinaryIDMap2{IndexBinaryFlat}  ("IBM2"/"IBxF")
 *   BINARY_IVF_FLAT -> IndexBinaryIVF, IndexBinaryFlat quantizer ("IBwF")
 * Save drops tombstoned rows; Flat rows keep arrival order, IVF rows are
 * grouped by list in arrival order; an untrained IVF index answers
 * DG_ENOT_SUPPORT.  Load also accepts "IBMp" and sparse ("sprs") list
 * sizes, keeps every IVF row in the list the file puts it in, answers
 * DG_ENOT_SUPPORT for any other fourcc (named in dg_last_error; every float
 * container is one), for a metric other than METRIC_L2
 * (vector_index_flat.cc:433-438) and for is_trained = 0, and DG_EIO for
 * malformed content.  The
 * file is read and checked completely before the first device call.  Byte
 * layout in DESIGN.md. */
dg_status dg_save_faiss_binary(dg_index* idx, const char* path);
dg_status dg_load_faiss_binary(dg_index** out, const char* path,
                               int32_t device);

/* ---- HNSW (DG_INDEX_HNSW; float vectors, L2 / IP / COSINE) ----
 * The graph is built on the host, one thread, by hnswlib's insertion
 * algorithm with a counter-based level draw (a build is a function of the
 * rows, their order and the seed); rows are held on the host as well as on
 * the device (the build reads them).  The graph is mirrored on the device
 * before the first search after a mutation and every search runs in one
 * kernel, one wave per query (HNSW, has the search definition).
 * dg_index_desc is unchanged: nlist, pq_m and pq_nbits are ignored.
 *  - defaults: nlinks 32, ef_construction 200, ef_search 10 (hnswlib's),
 *    seed 100 (vector_index_hnsw.cc:181-182).  dg_hnsw_configure only while
 *    the index is empty (else DG_EINVAL); nlinks 2..128 and ef_construction
 *    1..4096, else DG_ENOT_SUPPORT.
 *  - search: ef_search 0..1024 (vector_index_hnsw.cc:332), else DG_EINVAL;
 *    0 = the stored value (dg_hnsw_set_ef, 1..1024).  The beam is max(ef, k)
 *    wide.  k > 1024 is DG_ENOT_SUPPORT, k <= 0 an OK no-op, an empty index
 *    answers all -1.  Distances: L2 raw squared distance, IP / COSINE raw
 *    score; pads -1 / 0.0.  Every filter kind and negation apply.  dg_search
 *    / dg_search_device are dg_search_hnsw with ef_search = 0 (nprobe is
 *    ignored); dg_search_batched runs dg_search and counts the call as
 *    bypassed.  COSINE normalises rows and queries as the reference's HNSW
 *    does, x / (sqrtf(sum x^2) + 1e-30f), not with the 1e-5 window of the
 *    faiss kinds.  The _device form does not synchronise; a wave that meets
 *    a corrupt link or its iteration cap raises a flag that the host form,
 *    dg_hnsw_last_counters and dg_stats report as DG_EINTERNAL.
 *  - add / upsert / remove follow Flat: a negative id (DG_EINVAL), an id
 *    repeated in the call or (add) present (DG_EID_DUPLICATED), a NaN or
 *    infinite component (DG_EINVAL) and a remove with a missing id
 *    (DG_ENOT_FOUND) fail the whole call before anything moves.  Remove is
 *    hnswlib's markDelete: the node stays, is traversed, is never returned.
 *    Upsert of a present id marks the old node deleted and inserts a new
 *    one (hnswlib updates in place; the id answers with the new vector
 *    either way), so n_nodes grows with every upsert until a rebuild.
 *  - dg_train is an OK no-op, dg_reconstruct works, dg_add_device downloads
 *    the rows.  DG_ENOT_SUPPORT: dg_range_search, dg_save / dg_load,
 *    dg_save_faiss, dg_set_storage other than F32, dg_set_list_mask,
 *    dg_sharded_create.  The binary calls answer DG_EINVAL.
 *  - dg_stats: last_scan_ms is the search kernel's time (a batch so large
 *    that its visited bitmaps exceed 256 MB runs as several launches, and
 *    the clears of that workspace between them are then counted too),
 *    last_scan_bytes_algorithmic = dist_evals * 4 * d, device_bytes counts
 *    rows and graph.
 *  - dg_hnsw_export_* read the DEVICE copy back.  export_level: counts[i] =
 *    -1 where node i has no such level, links [n_nodes x cap(level)], cap =
 *    2 * nlinks on level 0 and nlinks above; level > max_level: DG_EINVAL.
 *  - dg_hnsw_last_counters: expansions (level-0 pops) and dist_evals (keys
 *    computed, on every level, the entry point's included) summed over the
 *    last search's batch; waits for the stream.
 *  - dg_save_hnswlib / dg_load_hnswlib: hnswlib's saveIndex container
 *    (0.7.x / 0.8.x layout), deleted nodes written with their
 *    mark.  The file carries neither metric nor d: the caller passes both
 *    (COSINE files hold normalised rows).  Malformed content is DG_EIO, an M
 *    outside 2..128 DG_ENOT_SUPPORT; the file is checked completely before
 *    the first device call. */
typedef struct dg_hnsw_info {
  int32_t nlinks, max_m0, ef_construction, ef_search, max_level;
  int64_t entry_point; /* internal node, -1 if empty */
  int64_t n_nodes;     /* tombstoned included */
  int64_t n_deleted;
  uint64_t seed;
} dg_hnsw_info;
dg_status dg_hnsw_configure(dg_index* idx, int32_t nlinks,
                            int32_t ef_construction, uint64_t seed);
dg_status dg_hnsw_set_ef(dg_index* idx, int32_t ef_search);
dg_status dg_hnsw_get_info(dg_index* idx, dg_hnsw_info* out);
dg_status dg_search_hnsw(dg_index* idx, int64_t nq, const float* x, int32_t k,
                         int32_t ef_search, const dg_filter* filter,
                         float* out_dist, int64_t* out_ids);
dg_status dg_search_hnsw_device(dg_index* idx, int64_t nq, const float* d_x,
                                int32_t k, int32_t ef_search,
                                const dg_filter* filter, float* d_out_dist,
                                int64_t* d_out_ids);
dg_status dg_hnsw_export_level(dg_index* idx, int32_t level, int32_t* counts,
                               uint32_t* links);
dg_status dg_hnsw_export_nodes(dg_index* idx, int64_t* ids, uint8_t* deleted,
                               int32_t* levels);
dg_status dg_hnsw_last_counters(dg_index* idx, int64_t* expansions,
                                int64_t* dist_evals);
dg_status dg_save_hnswlib(dg_index* idx, const char* path);
dg_status dg_load_hnswlib(dg_index** out, const char* path, int32_t metric,
                          int32_t d, int32_t device);
/* The container's max_elements field (hnswlib's capacity; this library grows
 * on demand and only carries the number): set >= 0 stores it, set < 0 only
 * reads.  Returns the stored value, 0 = "the node count at save"; -1 if idx
 * is not an HNSW index.  dg_load_hnswlib takes it from the file. */
int64_t dg_hnsw_max_elements(dg_index* idx, int64_t set);

/* ---- multi-GPU sharding support ----
 * Each rank holds a shard of the database (row-sharded)
 * with replicated centroids; local top-k is merged with an RCCL all-gather by
 * the caller.  An optional list mask restricts scanning to owned lists for
 * list-sharded deployments: mask[l] != 0 => list l is scanned here. */
dg_status dg_set_list_mask(dg_index* idx, const uint8_t* mask /* nlist */);

/* ---- merging best-first lists on the device ----
 * dists / ids are [n_lists][nq][k_in] result lists as dg_search returns
 * them (best first, padded with -1 / 0.0 behind the real rows); out is
 * [nq][k_out], the k_out best of each query's n_lists * k_in elements.
 * The order is strict and total: an element is smaller iff
 * (is_pad, key, list, pos) is lexicographically smaller, is_pad = id < 0,
 * key = the orderable image of the distance (L2) or of the negated score
 * (IP, COSINE; metric is a dg_metric), list / pos = where it stood in the
 * input.  -0.0 orders directly before +0.0 (for IP, score +0.0 before -0.0);
 * a real +inf distance still precedes every pad.  Every input list must be
 * sorted under that order, which the results of dg_search are.  Real
 * distances are copied bit for bit; pads, and the slots at or beyond
 * n_lists * k_in when k_out is larger, come out as -1 / 0.0f.
 * Limits: 1 <= n_lists <= 32, 1 <= k_in <= 2048, 1 <= k_out <= 2048
 * (DG_EINVAL otherwise).  This is the merge for results of sibling indexes,
 * for instance the regions of a split.
 * dg_merge_topk takes host pointers, runs on `device` (-1 = the current
 * one) and returns when out is written.  dg_merge_topk_device takes
 * pointers on the current device and enqueues on `stream` (a hipStream_t,
 * NULL = the default stream) without synchronising. */
dg_status dg_merge_topk(int32_t n_lists, int64_t nq, int32_t k_in,
                        int32_t k_out, int32_t metric, const float* dists,
                        const int64_t* ids, float* out_dist,
                        int64_t* out_ids, int32_t device);
dg_status dg_merge_topk_device(int32_t n_lists, int64_t nq, int32_t k_in,
                               int32_t k_out, int32_t metric,
                               const float* d_dists, const int64_t* d_ids,
                               float* d_out_dist, int64_t* d_out_ids,
                               void* stream);

/* ---- sharded index: one index over several GPUs of one process ----
 * A dg_sharded is n_shards ordinary indexes of one descriptor, one per
 * entry of devices[]; entries may repeat (several shards on one device is
 * legal: it is how the whole path runs on a single GPU).  Rows are routed by
 * id: shard = splitmix64(id) % n_shards, stateless, so an id always lives on
 * the same shard and ids are unique across shards.  Centroids and IVF-PQ
 * codebooks are replicated bit-identically, so every shard probes the same
 * lists.  A search fans out to every shard at the caller's k, gathers the
 * shards' lists into one slab on shard 0's device (the merge device) and
 * merges them there with the kernel behind dg_merge_topk.
 *
 *  - create: 1 <= n_shards <= 32 and valid device ordinals, else DG_EINVAL;
 *    devices = NULL puts every shard on device 0.  desc.device is ignored,
 *    desc.reserve is divided among the shards.  Float kinds only: a binary
 *    kind answers DG_ENOT_SUPPORT.  Every limit of dg_index_create holds per
 *    shard and is reported with that call's own error text; on any failure
 *    no shard is left alive.
 *  - train runs once, on shard 0 (already trained => OK no-op); its
 *    centroids, and for IVF-PQ its codebooks, are read back and installed on
 *    the other shards.  set_centroids / set_codebooks install on every
 *    shard, get_* read shard 0.
 *  - add / upsert / remove partition the rows on the host and hand every
 *    shard its part.  The all-or-nothing contracts hold for the whole call:
 *    a negative id (DG_EINVAL), an id twice in one call or (add) already
 *    present (DG_EID_DUPLICATED), an untrained index (DG_ENOT_TRAINED) and
 *    a remove with a missing id (DG_ENOT_FOUND) are answered before any
 *    shard is touched.  A device failure inside one shard is returned with
 *    that shard's message and is not rolled back on the others.
 *  - search has the semantics of dg_search: k <= 0 is an OK no-op, k > 2048
 *    DG_ENOT_SUPPORT, nprobe defaults and clamps per shard as in dg_search,
 *    an untrained IVF index returns all -1, padding is -1 / 0.0, a filter of
 *    any kind goes unchanged to every shard, cosine is normalised by the
 *    shards.  Ties between shards resolve toward the smaller shard.  The
 *    host form copies in and out and synchronises.  The _device form takes
 *    pointers on the merge device and enqueues the merge on the handle's
 *    merge stream; dg_sharded_sync waits for it.  Every shard's search is
 *    issued from its own worker thread (owned by the handle), so shards on
 *    different devices overlap.  A shard that fails returns its status and
 *    message; the other shards are drained, the merge is not run.
 *    Searches of one handle run one at a time.
 *  - range_search: every shard's dg_range_search, each query's rows
 *    concatenated on the host and sorted best-first, ties toward the smaller
 *    id (the order of dg_range_search); CSR results freed with dg_free.
 *  - stats: counts and bytes summed over the shards, stage times the maximum
 *    over the shards, the merge kernel's time added to last_select_ms.
 *  - dg_sharded_shard returns the borrowed dg_index of shard i (NULL if out
 *    of range) for inspection: dg_stats, dg_get_centroids, dg_export_assign.
 *    Mutating it directly breaks the routing.
 * Not offered: save / load of a sharded index (save the shards through
 * dg_sharded_shard, or rebuild), search batching, binary kinds, and the list
 * mask (the shards are row-sharded). */
typedef struct dg_sharded dg_sharded; /* opaque */
dg_status dg_sharded_create(dg_sharded** out, const dg_index_desc* desc,
                            int32_t n_shards, const int32_t* devices);
void dg_sharded_destroy(dg_sharded* sh);
dg_status dg_sharded_train(dg_sharded* sh, int64_t n, const float* x);
dg_status dg_sharded_set_centroids(dg_sharded* sh, int32_t nlist,
                                   const float* centroids);
dg_status dg_sharded_get_centroids(dg_sharded* sh, float* out_centroids);
dg_status dg_sharded_set_codebooks(dg_sharded* sh, int32_t m, int32_t nbits,
                                   const float* codebooks);
dg_status dg_sharded_get_codebooks(dg_sharded* sh, float* out_codebooks);
dg_status dg_sharded_add(dg_sharded* sh, int64_t n, const int64_t* ids,
                         const float* x);
dg_status dg_sharded_upsert(dg_sharded* sh, int64_t n, const int64_t* ids,
                            const float* x);
dg_status dg_sharded_remove(dg_sharded* sh, int64_t n, const int64_t* ids);
dg_status dg_sharded_search(dg_sharded* sh, int64_t nq, const float* x,
                            int32_t k, int32_t nprobe,
                            const dg_filter* filter,
                            float* out_dist /* nq x k */,
                            int64_t* out_ids /* nq x k */);
dg_status dg_sharded_search_device(dg_sharded* sh, int64_t nq,
                                   const float* d_x, int32_t k,
                                   int32_t nprobe, const dg_filter* filter,
                                   float* d_out_dist, int64_t* d_out_ids);
dg_status dg_sharded_sync(dg_sharded* sh);
dg_status dg_sharded_range_search(dg_sharded* sh, int64_t nq, const float* x,
                                  float radius, const dg_filter* filter,
                                  int64_t* lims /* nq+1 */,
                                  int64_t** out_ids, float** out_dists);
dg_status dg_sharded_stats(dg_sharded* sh, dg_stats_out* out);
int32_t dg_sharded_n_shards(dg_sharded* sh);
dg_index* dg_sharded_shard(dg_sharded* sh, int32_t i);
/* dg_set_storage on every shard, before any row is added (there is no
 * dg_sharded_reconstruct) */
dg_status dg_sharded_set_storage(dg_sharded* sh, int32_t storage);
/* dg_set_sq_ranges on every shard / dg_get_sq_ranges of shard 0.
 * dg_sharded_train replicates shard 0's ranges bit-identically, like its
 * centroids. */
dg_status dg_sharded_set_sq_ranges(dg_sharded* sh, const float* vmin,
                                   const float* vdiff);
dg_status dg_sharded_get_sq_ranges(dg_sharded* sh, float* vmin, float* vdiff);

/* ---- wrapper-lifecycle lock (LockWrite/UnlockWrite,
 * vector_index.h:192-193): the exclusive lock the reference wrapper takes
 * around its fork-save window; must be released by the same thread. ---- */
void dg_lock_write(dg_index* idx);
void dg_unlock_write(dg_index* idx);

/* ---- introspection ---- */
dg_status dg_stats(dg_index* idx, dg_stats_out* out);
void dg_last_error(char* buf, int64_t len);
/* 1 if the last IVF search that ran its kernels (not a graph replay) kept
 * the per-wave top-k inside the scan, 0 if it stored every candidate
 * (range search, IVF-PQ, large k, oversized slots, DG_SCAN_FUSED=0). */
int dg_last_scan_fused(dg_index* idx);
/* 1 if that fused scan ran the f32-MFMA kernel (the default), 0 if it ran
 * the VALU kernel (DG_SCAN_MFMA=0) or the search was not fused at all. */
int dg_last_scan_mfma(dg_index* idx);

/* 1 if the last search also launched the pair scan (k_ivf_scan_mfma2: lists
 * probed by 17 or more queries are scanned two 16-query tiles per pass), 0
 * if k_ivf_scan_mfma took every tile: DG_SCAN_PAIR=0, no more than 16
 * queries, d > 2304, or not the f32-MFMA scan at all. */
int dg_last_scan_pair(dg_index* idx);
/* 1 if the last IVF-Flat search that ran its kernels scanned f16 rows
 * (k_ivf_scan_f16, either candidate flow), 0 otherwise. */
int dg_last_scan_f16(dg_index* idx);
/* 1 if the last IVF-Flat search that ran its kernels scanned SQ8 rows
 * (k_ivf_scan_sq8, either candidate flow), 0 otherwise. */
int dg_last_scan_sq8(dg_index* idx);
/* 1 if the last IVF search that ran its kernels (any IVF kind) selected its
 * probes with the one-kernel radix select (k_coarse_select), 0 if it ran
 * k_select_dense + k_probe_unpack: DG_COARSE_WAVE=0, nprobe > 128, or
 * nprobe >= nlist (every list probed, nothing selected). */
int dg_last_coarse_wave(dg_index* idx);
/* Debugging accessor: the probes of the last IVF search, [nq][nprobe] list
 * ids in selection order (best first), -1 where the list mask removed one.
 * Waits for the index's stream, copies min(n, nq * nprobe) entries to the
 * host array out and returns nq * nprobe (so n = 0, out = NULL asks for the
 * size); 0 before the first IVF search, -1 on error. */
int64_t dg_last_probes(dg_index* idx, int32_t* out, int64_t n);
int dg_device_count(void);
/* Library self-identification: returns a static string with build arch. */
const char* dg_build_info(void);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* DINGO_GPU_H_ */
