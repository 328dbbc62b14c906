// vector_index_gpu.h — C++ mirror of dingo-store's VectorIndex plugin
// surface (reference: src/vector/vector_index.h:56-279) implemented on top
// of the C-ABI in include/dingo_gpu.h.  A dingo-store maintainer drops this
// subclass into the Index role by registering it in VectorIndexFactory::New
// (src/vector/vector_index_factory.cc:40-95) — see INTEGRATION.md for the
// exact stub.  Proto schemas are absent from the reference tree
// (dingo-store-proto is an empty submodule), so the boundary types below are
// plain-struct re-declarations reconstructed from the call sites cited in
// SURVEY.md §3.1/§8b.
#pragma once

#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/dingo_gpu.h"

namespace dingogpu {

// ---- pb::common::* re-declarations (schema absent; field set from call
// sites, e.g. ExtractVectorValue src/vector/vector_index_utils.cc:564-609,
// FillSearchResult :612-655) ----
enum class MetricType {
  kL2 = 0,
  kInnerProduct = 1,
  kCosine = 2,
  kHamming = 3  // binary indexes only
};
enum class ValueType { kFloat = 0, kUint8 = 1 };

struct Vector {
  int32_t dimension = 0;
  ValueType value_type = ValueType::kFloat;
  std::vector<float> float_values;
  // ValueType::kUint8: dimension / 8 packed bytes (binary indexes)
  std::vector<uint8_t> binary_values;
};

struct VectorWithId {
  int64_t id = -1;
  Vector vector;
};

struct VectorWithDistance {
  VectorWithId vector_with_id;
  float distance = 0.f;  // dingo convention: L2 raw sqr; IP/cos 1 - score
  MetricType metric_type = MetricType::kL2;
};

struct VectorWithDistanceResult {
  std::vector<VectorWithDistance> vector_with_distances;
};

struct VectorSearchParameter {
  int32_t top_n = 0;
  bool use_brute_force = false;
  bool without_vector_data = true;
  int32_t ivf_flat_nprobe = 0;  // parameter.ivf_flat().nprobe()
  int32_t ivf_pq_nprobe = 0;
  int32_t binary_ivf_flat_nprobe = 0;  // parameter.binary_ivf_flat().nprobe()
  int32_t hnsw_efsearch = 0;  // parameter.hnsw().efsearch(); 0 = the index's
  bool enable_range_search = false;
  float radius = 0.f;
};

// butil::Status analog (pb::error::Errno codes preserved numerically where
// the reader dispatches on them)
struct Status {
  int code = 0;  // 0 = OK
  std::string msg;
  bool ok() const { return code == 0; }
  static Status OK() { return {}; }
};
// Errno values the reader dispatches on (reference pb/error.proto usage):
constexpr int kEillegalParamteters = 30001;  // EILLEGAL_PARAMTETERS
constexpr int kEVectorNotTrain = 30008;      // triggers train-first handling
constexpr int kEVectorNotSupport = 30010;    // reader brute-force fallback
constexpr int kEVectorIdDuplicated = 30011;
constexpr int kEVectorInvalid = 30012;
constexpr int kEInternal = 10002;

// ---- FilterFunctor mirror (vector_index.h:67-146) ----
class FilterFunctor {
 public:
  virtual ~FilterFunctor() = default;
  // hook the reference gives filters to pre-index the id universe
  // (vector_index.h:70); default no-op like the reference
  virtual void Build(std::vector<int64_t>& /*id_map*/) {}
  virtual bool Check(int64_t vector_id) = 0;
  // translate to the device filter; default: unsupported (caller falls back
  // to post-filtering like the reader's over-fetch path)
  virtual bool ToDeviceFilter(dg_filter* out) const { return false; }
};

class RangeFilterFunctor : public FilterFunctor {  // vector_index.h:77-84
 public:
  RangeFilterFunctor(int64_t min_id, int64_t max_id)
      : min_(min_id), max_(max_id) {}
  bool Check(int64_t id) override { return id >= min_ && id < max_; }
  bool ToDeviceFilter(dg_filter* out) const override {
    *out = {};
    out->kind = DG_FILTER_RANGE;
    out->min_id = min_;
    out->max_id = max_;
    return true;
  }

 private:
  int64_t min_, max_;
};

class SortFilterFunctor : public FilterFunctor {  // vector_index.h:109-146
 public:
  explicit SortFilterFunctor(std::vector<int64_t> ids, bool negation = false)
      : ids_(std::move(ids)), negation_(negation) {}
  bool Check(int64_t id) override;
  bool ToDeviceFilter(dg_filter* out) const override {
    *out = {};
    out->kind = DG_FILTER_SORTED_IDS;
    out->ids = ids_.data();
    out->n_ids = (int64_t)ids_.size();
    out->negate = negation_ ? 1 : 0;
    return true;
  }

 private:
  std::vector<int64_t> ids_;
  bool negation_;
};

// ConcreteFilterFunctor mirror (vector_index.h:86-106: faiss IDSelectorBatch
// membership + optional negation); device form = sorted-id filter
class ConcreteFilterFunctor : public FilterFunctor {
 public:
  explicit ConcreteFilterFunctor(const std::vector<int64_t>& ids,
                                 bool is_negation = false);
  bool Check(int64_t id) override;
  bool ToDeviceFilter(dg_filter* out) const override {
    *out = {};
    out->kind = DG_FILTER_SORTED_IDS;
    out->ids = sorted_.data();
    out->n_ids = (int64_t)sorted_.size();
    out->negate = negation_ ? 1 : 0;
    return true;
  }

 private:
  std::vector<int64_t> sorted_;
  bool negation_;
};

// ---- VectorIndex mirror (vector_index.h:148-229 virtuals; every
// must-implement virtual the wrapper/manager calls is present) ----
class VectorIndex {
 public:
  virtual ~VectorIndex() = default;
  virtual int32_t GetDimension() = 0;
  virtual MetricType GetMetricType() = 0;
  virtual Status GetCount(int64_t& count) = 0;
  virtual Status GetDeletedCount(int64_t& deleted_count) = 0;
  virtual Status GetMemorySize(int64_t& bytes) = 0;
  virtual bool IsExceedsMaxElements(int64_t vector_size) = 0;
  virtual Status Add(const std::vector<VectorWithId>& v) = 0;
  virtual Status Upsert(const std::vector<VectorWithId>& v) = 0;
  virtual Status Delete(const std::vector<int64_t>& ids) = 0;
  virtual Status Train(const std::vector<VectorWithId>& v) = 0;
  // raw float form (vector_index.h:196: Train(std::vector<float>&))
  virtual Status Train(std::vector<float>& train_datas) = 0;
  virtual bool IsTrained() = 0;
  virtual bool NeedTrain() = 0;
  // rebuild/save scheduling hooks VectorIndexManager drives
  // (vector_index.h:198-204; semantics per concrete index)
  virtual bool NeedToRebuild() = 0;
  virtual bool NeedToSave(int64_t last_save_log_behind) = 0;
  virtual bool SupportSave() { return false; }
  // exclusive lock for the wrapper's fork-save window
  // (vector_index.h:192-193; rw_lock_.LockWrite/UnlockWrite)
  virtual void LockWrite() = 0;
  virtual void UnlockWrite() = 0;
  virtual Status Save(const std::string& path) = 0;
  virtual Status Load(const std::string& path) = 0;
  virtual Status Search(const std::vector<VectorWithId>& queries,
                        uint32_t topk,
                        const std::vector<std::shared_ptr<FilterFunctor>>& f,
                        bool reconstruct, const VectorSearchParameter& p,
                        std::vector<VectorWithDistanceResult>& results) = 0;
  virtual Status RangeSearch(
      const std::vector<VectorWithId>& queries, float radius,
      const std::vector<std::shared_ptr<FilterFunctor>>& f, bool reconstruct,
      const VectorSearchParameter& p,
      std::vector<VectorWithDistanceResult>& results) = 0;
};

// ---- reader brute-force fallback ----
// Mirror of VectorReader::BruteForceSearch (vector_reader.cc:1873-2048):
// scan the region's rows in FLAGS_vector_index_bruteforce_batch_count
// batches (default 2048, vector_reader.cc:61), build a throwaway Flat
// index per batch, search it, and merge per-query top-k by the dingo
// distance (max-heap keeps the smallest topk; output ascending).  The KV
// iterator is abstracted as a pull function (the real reader wires the
// RocksDB range scan + proto decode here, vector_reader.cc:1922-1936).
using RowIterator = std::function<bool(VectorWithId*)>;

Status BruteForceSearch(MetricType metric, int32_t dimension,
                        const RowIterator& next,
                        const std::vector<VectorWithId>& queries,
                        uint32_t topk,
                        const std::vector<std::shared_ptr<FilterFunctor>>& f,
                        const VectorSearchParameter& p,
                        std::vector<VectorWithDistanceResult>& results,
                        int64_t batch_count = 2048);

// Search with the reader's EVECTOR_NOT_SUPPORT fallback round trip
// (vector_reader.cc:1828-1831): an index that rejects the request drops
// to the KV-scan brute force.  scan_factory yields a fresh iterator.
Status SearchWithBruteForceFallback(
    VectorIndex* index, const std::function<RowIterator()>& scan_factory,
    const std::vector<VectorWithId>& queries, uint32_t topk,
    const std::vector<std::shared_ptr<FilterFunctor>>& f,
    const VectorSearchParameter& p,
    std::vector<VectorWithDistanceResult>& results);

// GPU-backed concrete indexes (Flat / IVF-Flat), the factory, and a
// self-test used by the GPU test suite.
std::unique_ptr<VectorIndex> NewFlatIndex(MetricType metric, int32_t dim,
                                          int device = -1);
std::unique_ptr<VectorIndex> NewIvfFlatIndex(MetricType metric, int32_t dim,
                                             int32_t ncentroids,
                                             int device = -1);
// IVF-Flat whose rows are stored as IEEE halves (dg_set_storage,
// DG_STORAGE_F16): half the device memory and half the bytes per search;
// distances are those between the f32 query and the rounded row.  Add and
// Upsert fail with EILLEGAL_PARAMTETERS on a component that is NaN or above
// 65504 in magnitude.  Save and Load use the library's own container
// (dg_save / dg_load), which no CPU node reads; Load refuses a file of
// another kind, dimension, metric or storage.
std::unique_ptr<VectorIndex> NewIvfFlatIndexF16(MetricType metric, int32_t dim,
                                                int32_t ncentroids,
                                                int device = -1);
// IVF-Flat whose rows are stored as one byte per component (dg_set_storage,
// DG_STORAGE_SQ8: the codec of faiss QT_8bit): a quarter of the device
// memory and of the bytes per search; distances are those between the f32
// query and the decoded row.  Train yields the per-dimension ranges (min and
// max - min of the training rows) next to the centroids, and IsTrained needs
// both.  A component outside its range saturates; Add and Upsert fail with
// EILLEGAL_PARAMTETERS on a NaN or infinite component.  Save and Load as for
// NewIvfFlatIndexF16.
std::unique_ptr<VectorIndex> NewIvfFlatIndexSq8(MetricType metric, int32_t dim,
                                                int32_t ncentroids,
                                                int device = -1);
std::unique_ptr<VectorIndex> NewIvfPqIndex(MetricType metric, int32_t dim,
                                           int32_t ncentroids,
                                           int32_t nsubvector,
                                           int device = -1);
// The same with nbits_per_idx, normalised like the reference (% 64, 0 -> 8;
// vector_index_ivf_pq.cc:64-66).  The GPU library runs 4 and 8 (4 packs two
// codes per byte and needs nsubvector % 8 == 0); for any other value, or a
// geometry it refuses, the returned index answers EVECTOR_NOT_SUPPORT to
// every call, so SearchWithBruteForceFallback takes the reader's scan.
std::unique_ptr<VectorIndex> NewIvfPqIndex(MetricType metric, int32_t dim,
                                           int32_t ncentroids,
                                           int32_t nsubvector,
                                           int32_t nbits_per_idx, int device);

// Binary (Hamming) indexes: dim in bits, vectors carry binary_values of
// dim / 8 bytes; distances are the integer Hamming distance, passed through
// (vector_index_utils.cc:640-650).  RangeSearch truncates its float radius
// to faiss's int (a row is returned iff hamming < radius) and reads nprobe
// from binary_ivf_flat_nprobe; Save/Load speak the faiss write_index_binary
// container, and Load refuses a file of another kind or dimension, or (IVF)
// of an nlist that is neither the index's current nor its configured one.
std::unique_ptr<VectorIndex> NewBinaryFlatIndex(int32_t dim, int device = -1);
std::unique_ptr<VectorIndex> NewBinaryIvfFlatIndex(int32_t dim,
                                                   int32_t ncentroids,
                                                   int device = -1);

// HNSW (VectorIndexHnsw, vector_index_hnsw.cc): a host-built graph searched
// on the GPU, metric L2 / inner product / cosine.  Add is Upsert, Delete of a
// missing id is EINTERNAL, Delete marks (hnswlib markDelete) and an Upsert of
// a present id marks the old node and inserts a new one, so the element count
// behind IsExceedsMaxElements (count + vector_size > max_elements) and
// NeedToRebuild (deleted above half of it) includes marked nodes.  Search
// reads hnsw_efsearch (0..1024, else EILLEGAL_PARAMTETERS; 0 = the index's
// stored value) and fills float_values when reconstruct is set; RangeSearch
// answers EVECTOR_NOT_SUPPORT.  Save / Load speak hnswlib's saveIndex
// container; Load takes metric and dimension from this index.  nullptr if
// the library refuses the parameters (nlinks 2..128, efconstruction 1..4096).
std::unique_ptr<VectorIndex> NewHnswIndex(MetricType metric, int32_t dim,
                                          int32_t nlinks,
                                          int32_t efconstruction,
                                          int64_t max_elements,
                                          int device = -1);

// Search batching (off by default).  The reference's search pool calls
// Search from 16 threads with one query each (vector_index.cc:53-54,244-271)
// and one index runs one search at a time.  With batching on, Search of a
// GPU index (float and binary kinds) goes through dg_search_batched /
// dg_search_binary_batched, which merge the waiting calls into one device
// batch; every call still returns its own rows (include/dingo_gpu.h, "search
// batching").  max_batch 0 = 64 queries; max_wait_us 0 = a batch never waits
// for company once the device is free.  Call it before the index is handed
// to the pool; the setting survives Load.  EVECTOR_NOT_SUPPORT for an index
// that is not GPU-backed.  RangeSearch is not batched.
Status EnableBatching(VectorIndex* index, int32_t max_batch = 0,
                      int32_t max_wait_us = 0);
Status DisableBatching(VectorIndex* index);

// One index sharded over several GPUs of this process (dg_sharded_*,
// include/dingo_gpu.h): devices holds one HIP ordinal per shard (1 to 32
// entries; an ordinal may repeat, which puts several shards on one device).
// Rows are routed to shards by id, Search fans out to all of them and merges
// on the first shard's device; the surface, the 1 - score flip and the error
// mapping are those of the single-device indexes.  Save and Load answer
// EVECTOR_NOT_SUPPORT (SupportSave() is false), LockWrite / UnlockWrite are
// no-ops (the handle locks inside) and search batching is not offered.
// nullptr if the library refuses the parameters.
std::unique_ptr<VectorIndex> NewShardedFlatIndex(MetricType metric,
                                                 int32_t dim,
                                                 std::vector<int> devices);
std::unique_ptr<VectorIndex> NewShardedIvfFlatIndex(MetricType metric,
                                                    int32_t dim,
                                                    int32_t ncentroids,
                                                    std::vector<int> devices);
std::unique_ptr<VectorIndex> NewShardedIvfPqIndex(MetricType metric,
                                                  int32_t dim,
                                                  int32_t ncentroids,
                                                  int32_t nsubvector,
                                                  int32_t nbits_per_idx,
                                                  std::vector<int> devices);

}  // namespace dingogpu

extern "C" {
// Runs a tiny Flat + IVF search through the C++ plugin mirror on the GPU and
// verifies the dingo-store observable semantics (1 - score flip for
// IP/cosine, vector_index_utils.cc:634; self-top-1).  Returns 0 on success.
int dg_mirror_selftest(void);
// Same for the binary indexes: Flat and IVF-Flat through the mirror, self
// top-1 at distance 0 and the Hamming distance passed through unflipped,
// range search against a host popcount, Save -> Load -> the same top-4.
int dg_mirror_selftest_binary(void);
// IVF-PQ at nbits_per_idx = 4 through the mirror: Train -> Add -> self top-1
// -> Save -> Load -> the same top-4; an unsupported nbits_per_idx answers
// EVECTOR_NOT_SUPPORT and the brute-force fallback serves the search.
int dg_mirror_selftest_pq4(void);
// Search batching through the mirror, the reference pool's call shape: 16
// std::threads, one query per Search, on an L2 IVF-Flat index without and
// with a RangeFilterFunctor, an inner-product Flat index (the 1 - score
// flip) and a binary Flat index.  Every answer is compared with the same
// call made before batching was enabled: the same ids, float distances
// within 1e-4 relative, binary distances equal.  Batches must have formed.
int dg_mirror_selftest_batched(void);
// 2-shard Flat indexes (both shards on device 0) through the mirror, L2 and
// inner product, on rows whose distances are exact in float32: the merged
// order, the 1 - score flip, pads skipped at k above the row count, Delete /
// Add / Upsert contracts across shards, Save / Load not supported.
int dg_mirror_selftest_sharded(void);
// NewIvfFlatIndexF16 through the mirror, on rows that are exact in half:
// Train -> Add -> self top-1 at distance 0 -> an Add with a component above
// 65504 refused, the count unchanged -> Save -> Load into a fresh f16 index
// -> the same top-4, bit for bit.
int dg_mirror_selftest_f16(void);
// NewIvfFlatIndexSq8 through the mirror: an Add before Train refused ->
// Train (centroids and ranges) -> Add -> self top-1 within half a step per
// dimension -> an Add with a NaN component refused, the count unchanged ->
// Save -> Load into a fresh SQ8 index (an f16 index refuses the file) -> the
// same top-4, bit for bit.
int dg_mirror_selftest_sq8(void);
// NewHnswIndex through the mirror, L2 and inner product: Add (an Upsert) ->
// counts and the max-elements / save / rebuild rules -> self top-1 at
// distance 0 with the stored vector returned, the 1 - score flip -> a range
// filter -> the efsearch bound -> Delete contracts -> Save -> Load (a wrong
// dimension refused) -> the same top-4, bit for bit.
int dg_mirror_selftest_hnsw(void);
// The second driver of tools/bench_concurrent.py, free of Python threads:
// `threads` std::threads search the rows of q ([nq x d] float32) round-robin
// through dg_search (batched = 0) or dg_search_batched, one query per call,
// `calls_per_thread` times each.  Returns the wall time in seconds, < 0 on
// an error.
double dg_bench_threads(dg_index* idx, int32_t threads,
                        int32_t calls_per_thread, int32_t batched,
                        const float* q, int64_t nq, int32_t k,
                        int32_t nprobe);
}
