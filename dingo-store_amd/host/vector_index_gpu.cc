// vector_index_gpu.cc — GPU-backed implementations of the VectorIndex
// plugin mirror.  Thin shim over the C-ABI: marshals the plain-struct proto
// re-declarations to packed arrays (restating ExtractVectorValue,
// src/vector/vector_index_utils.cc:564-609) and shapes results exactly like
// FillSearchResult (:612-655): L2 raw squared distance passes through,
// IP/cosine reported as 1.0f - score (:634), labels < 0 skipped.
#include "vector_index_gpu.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <queue>
#include <thread>
#include <unordered_set>

#include <unistd.h>

namespace dingogpu {

ConcreteFilterFunctor::ConcreteFilterFunctor(const std::vector<int64_t>& ids,
                                             bool is_negation)
    : sorted_(ids), negation_(is_negation) {
  std::sort(sorted_.begin(), sorted_.end());
  sorted_.erase(std::unique(sorted_.begin(), sorted_.end()), sorted_.end());
}

bool ConcreteFilterFunctor::Check(int64_t id) {
  bool found = std::binary_search(sorted_.begin(), sorted_.end(), id);
  return negation_ ? !found : found;
}

bool SortFilterFunctor::Check(int64_t id) {
  int64_t lo = 0, hi = (int64_t)ids_.size() - 1;
  bool found = false;
  while (lo <= hi) {  // binary search, vector_index.h:117-133
    int64_t mid = (lo + hi) / 2;
    if (ids_[mid] == id) {
      found = true;
      break;
    }
    if (id < ids_[mid]) hi = mid - 1; else lo = mid + 1;
  }
  return negation_ ? !found : found;
}

namespace {

Status from_dg(dg_status st) {
  if (st == DG_OK) return Status::OK();
  char buf[512];
  dg_last_error(buf, sizeof(buf));
  int code;
  switch (st) {
    case DG_EINVAL: code = kEillegalParamteters; break;
    case DG_ENOT_TRAINED: code = kEVectorNotTrain; break;
    case DG_ENOT_SUPPORT: code = kEVectorNotSupport; break;
    case DG_EID_DUPLICATED: code = kEVectorIdDuplicated; break;
    case DG_ENOT_FOUND: code = kEVectorInvalid; break;
    default: code = kEInternal; break;
  }
  return {code, buf};
}

// pack VectorWithId batch -> contiguous floats + ids, checking dimensions
// (CheckVectorDimension semantics, utils.cc; normalization happens inside
// the library for cosine)
Status pack(const std::vector<VectorWithId>& v, int32_t dim,
            std::vector<float>& x, std::vector<int64_t>& ids) {
  x.resize((size_t)v.size() * dim);
  ids.resize(v.size());
  for (size_t i = 0; i < v.size(); i++) {
    if ((int32_t)v[i].vector.float_values.size() != dim)
      return {kEillegalParamteters, "dimension not match"};
    memcpy(&x[i * dim], v[i].vector.float_values.data(),
           (size_t)dim * sizeof(float));
    ids[i] = v[i].id;
  }
  return Status::OK();
}

// binary form: binary_values of dim / 8 bytes each; a size mismatch is
// EVECTOR_INVALID (utils.cc:512)
Status pack_bits(const std::vector<VectorWithId>& v, int32_t dim,
                 std::vector<uint8_t>& x, std::vector<int64_t>& ids) {
  const size_t rb = (size_t)dim / 8;
  x.resize(v.size() * rb);
  ids.resize(v.size());
  for (size_t i = 0; i < v.size(); i++) {
    if (v[i].vector.binary_values.size() != rb)
      return {kEVectorInvalid, "binary dimension not match"};
    memcpy(&x[i * rb], v[i].vector.binary_values.data(), rb);
    ids[i] = v[i].id;
  }
  return Status::OK();
}

class GpuIndexBase : public VectorIndex {
 public:
  GpuIndexBase(dg_index_kind kind, MetricType metric, int32_t dim,
               int32_t nlist, int device, int32_t pq_m = 0,
               int32_t pq_nbits = 8) {
    metric_ = metric;
    dim_ = dim;
    binary_ = kind == DG_INDEX_BINARY_FLAT || kind == DG_INDEX_BINARY_IVF_FLAT;
    dg_index_desc desc{};
    desc.kind = (int32_t)kind;
    desc.metric = (int32_t)metric;
    desc.d = dim;
    desc.nlist = nlist;
    desc.pq_m = pq_m;
    desc.pq_nbits = pq_nbits;
    desc.device = device;
    create_st_ = dg_index_create(&idx_, &desc);
    dg_stats_out s{};
    if (create_st_ == DG_OK && dg_stats(idx_, &s) == DG_OK)
      nlist_created_ = s.nlist;  // after the defaults of dg_index_create
  }
  ~GpuIndexBase() override {
    if (idx_) dg_index_destroy(idx_);
  }
  Status CreateStatus() const { return from_dg(create_st_); }

  int32_t GetDimension() override { return dim_; }
  MetricType GetMetricType() override { return metric_; }
  Status GetCount(int64_t& count) override {
    dg_stats_out s{};
    dg_status st = dg_stats(idx_, &s);
    count = s.ntotal;
    return from_dg(st);
  }
  Status GetMemorySize(int64_t& bytes) override {
    dg_stats_out s{};
    dg_status st = dg_stats(idx_, &s);
    bytes = s.device_bytes;
    return from_dg(st);
  }
  Status Add(const std::vector<VectorWithId>& v) override {
    if (v.empty()) return {kEillegalParamteters, "vector_with_ids is empty"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    if (binary_) {
      std::vector<uint8_t> b;
      Status s = pack_bits(v, dim_, b, ids);
      if (!s.ok()) return s;
      return from_dg(
          dg_add_binary(idx_, (int64_t)v.size(), ids.data(), b.data()));
    }
    Status s = pack(v, dim_, x, ids);
    if (!s.ok()) return s;
    return from_dg(dg_add(idx_, (int64_t)v.size(), ids.data(), x.data()));
  }
  Status Upsert(const std::vector<VectorWithId>& v) override {
    if (v.empty()) return {kEillegalParamteters, "vector_with_ids is empty"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    if (binary_) {
      std::vector<uint8_t> b;
      Status s = pack_bits(v, dim_, b, ids);
      if (!s.ok()) return s;
      return from_dg(
          dg_upsert_binary(idx_, (int64_t)v.size(), ids.data(), b.data()));
    }
    Status s = pack(v, dim_, x, ids);
    if (!s.ok()) return s;
    return from_dg(dg_upsert(idx_, (int64_t)v.size(), ids.data(), x.data()));
  }
  Status Delete(const std::vector<int64_t>& ids) override {
    if (ids.empty()) return {kEillegalParamteters, "empty ids"};
    return from_dg(dg_remove(idx_, (int64_t)ids.size(), ids.data()));
  }
  Status Train(const std::vector<VectorWithId>& v) override {
    if (v.empty()) return {kEillegalParamteters, "data size invalid"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    Status s;
    if (binary_) {
      std::vector<uint8_t> b;
      s = pack_bits(v, dim_, b, ids);
      if (!s.ok()) return s;
      s = from_dg(dg_train_binary(idx_, (int64_t)v.size(), b.data()));
    } else {
      s = pack(v, dim_, x, ids);
      if (!s.ok()) return s;
      s = from_dg(dg_train(idx_, (int64_t)v.size(), x.data()));
    }
    if (s.ok()) train_data_size_ = (int64_t)v.size();
    return s;
  }
  Status Train(std::vector<float>& train_datas) override {
    // raw-float Train (vector_index.h:196; size checks per
    // vector_index_ivf_flat.cc:644-652)
    if (binary_)
      return {kEVectorNotSupport, "raw-float train on a binary index"};
    size_t data_size = train_datas.size() / dim_;
    if (data_size == 0)
      return {kEillegalParamteters, "data size invalid"};
    if (train_datas.size() % dim_ != 0)
      return {kEillegalParamteters, "dimension not match"};
    Status s = from_dg(dg_train(idx_, (int64_t)data_size,
                                train_datas.data()));
    if (s.ok()) train_data_size_ = (int64_t)data_size;
    return s;
  }
  bool IsTrained() override {
    dg_stats_out s{};
    return dg_stats(idx_, &s) == DG_OK && s.is_trained;
  }
  Status GetDeletedCount(int64_t& deleted_count) override {
    // the reference's faiss path compacts on remove and reports 0
    // (vector_index_ivf_flat.cc:539-542); here removes tombstone until the
    // next finalize, so the pending count is reported
    dg_stats_out s{};
    dg_status st = dg_stats(idx_, &s);
    deleted_count = s.deleted_count;
    return from_dg(st);
  }
  bool IsExceedsMaxElements(int64_t) override {
    return false;  // flat.cc:510-512, ivf_flat.cc:573-575
  }
  bool NeedToRebuild() override { return false; }  // per-kind overrides
  bool NeedToSave(int64_t last_save_log_behind) override {
    // flat.cc:515-531 / ivf_flat.cc:786-800: trained, non-empty, and the
    // raft log has run ahead of the last snapshot by > need_save_count
    // (DEFINE_int64(..._need_save_count, 10000) in all three indexes)
    dg_stats_out s{};
    if (dg_stats(idx_, &s) != DG_OK) return false;
    if (!s.is_trained || s.ntotal == 0) return false;
    return last_save_log_behind > kNeedSaveCount;
  }
  bool SupportSave() override { return true; }
  void LockWrite() override { dg_lock_write(idx_); }
  void UnlockWrite() override { dg_unlock_write(idx_); }
  Status Save(const std::string& path) override {
    if (binary_) return from_dg(dg_save_faiss_binary(idx_, path.c_str()));
    // the snapshot cycle ships faiss::write_index files
    // (vector_index_snapshot_manager.cc:583-599) — emit the compatible
    // container so CPU nodes can ingest the snapshot
    return from_dg(dg_save_faiss(idx_, path.c_str()));
  }
  Status Load(const std::string& path) override {
    dg_index* ni = nullptr;
    dg_status st =
        binary_ ? dg_load_faiss_binary(&ni, path.c_str(), -1)
                : dg_load_faiss(&ni, path.c_str(), (int32_t)metric_, -1);
    if (st != DG_OK) return from_dg(st);
    if (binary_) {
      // the file must hold this index's kind and dimension (the reference's
      // dynamic_cast and "dimension not match", vector_index_flat.cc:389-406)
      dg_stats_out now{}, got{};
      // and, for IVF, its current or its configured nlist
      // (vector_index_ivf_flat.cc:495-498)
      if (dg_stats(idx_, &now) != DG_OK || dg_stats(ni, &got) != DG_OK ||
          got.kind != now.kind || got.d != dim_ ||
          (got.kind == DG_INDEX_BINARY_IVF_FLAT && got.nlist != now.nlist &&
           got.nlist != nlist_created_)) {
        dg_index_destroy(ni);
        return {kEInternal, "loaded index kind, dimension or nlist not match"};
      }
    }
    dg_index_destroy(idx_);
    idx_ = ni;
    // batching belongs to the dg_index: carry it over to the loaded one
    if (batching_) return EnableBatching(batch_opts_.max_batch,
                                         batch_opts_.max_wait_us);
    return Status::OK();
  }

  // Search then goes through dg_search_batched / dg_search_binary_batched,
  // which merge the pool's concurrent one-query calls into device batches
  Status EnableBatching(int32_t max_batch, int32_t max_wait_us) {
    batch_opts_.max_batch = max_batch;
    batch_opts_.max_wait_us = max_wait_us;
    dg_status st = dg_batching_enable(idx_, &batch_opts_);
    batching_ = st == DG_OK;
    return from_dg(st);
  }
  Status DisableBatching() {
    batching_ = false;
    return from_dg(dg_batching_disable(idx_));
  }
  Status BatchingStats(dg_batch_stats* out) {
    return from_dg(dg_batching_stats(idx_, out));
  }

  Status Search(const std::vector<VectorWithId>& queries, uint32_t topk,
                const std::vector<std::shared_ptr<FilterFunctor>>& filters,
                bool, const VectorSearchParameter& p,
                std::vector<VectorWithDistanceResult>& results) override {
    // mirrors VectorIndexFlat/IvfFlat::Search argument handling
    // (vector_index_flat.cc:205-221, ivf_flat.cc:191-236)
    if (queries.empty())
      return {kEillegalParamteters, "vector_with_ids is empty"};
    if (topk == 0) return Status::OK();
    std::vector<float> x;
    std::vector<uint8_t> xb;
    std::vector<int64_t> ids;
    Status s = binary_ ? pack_bits(queries, dim_, xb, ids)
                       : pack(queries, dim_, x, ids);
    if (!s.ok()) return s;

    dg_filter df{};
    dg_filter* dfp = nullptr;
    if (!filters.empty()) {
      // one translatable filter supported natively; otherwise the reader's
      // post-filter path applies (not replicated here)
      if (filters.size() == 1 && filters[0]->ToDeviceFilter(&df)) {
        dfp = &df;
      } else {
        return {kEVectorNotSupport, "composite filters via reader fallback"};
      }
    }
    int32_t nprobe = binary_ ? p.binary_ivf_flat_nprobe : p.ivf_flat_nprobe;
    std::vector<float> dist((size_t)queries.size() * topk);
    std::vector<int64_t> labels((size_t)queries.size() * topk, -1);
    const auto search_f = batching_ ? dg_search_batched : dg_search;
    const auto search_b =
        batching_ ? dg_search_binary_batched : dg_search_binary;
    dg_status st =
        binary_ ? search_b(idx_, (int64_t)queries.size(), xb.data(),
                           (int32_t)topk, nprobe, dfp, dist.data(),
                           labels.data())
                : search_f(idx_, (int64_t)queries.size(), x.data(),
                           (int32_t)topk, nprobe, dfp, dist.data(),
                           labels.data());
    if (st != DG_OK) return from_dg(st);
    // FillSearchResult shaping (utils.cc:612-655)
    results.clear();
    results.resize(queries.size());
    for (size_t row = 0; row < queries.size(); row++) {
      for (uint32_t i = 0; i < topk; i++) {
        size_t pos = row * topk + i;
        if (labels[pos] < 0) continue;  // padding skipped, :622-624
        VectorWithDistance vd;
        vd.vector_with_id.id = labels[pos];
        vd.vector_with_id.vector.dimension = dim_;
        vd.metric_type = metric_;
        // L2 and Hamming (:640-650) pass through; IP/cosine flip, :634
        vd.distance = (metric_ == MetricType::kL2 ||
                       metric_ == MetricType::kHamming)
                          ? dist[pos]
                          : 1.0f - dist[pos];
        results[row].vector_with_distances.push_back(std::move(vd));
      }
    }
    return Status::OK();
  }

  Status RangeSearch(const std::vector<VectorWithId>& queries, float radius,
                     const std::vector<std::shared_ptr<FilterFunctor>>& fs,
                     bool, const VectorSearchParameter& p,
                     std::vector<VectorWithDistanceResult>& results) override {
    // mirrors VectorIndexIvfFlat::RangeSearch: for IP/cosine the dingo
    // radius converts to a faiss score threshold 1 - r
    // (src/vector/vector_index_ivf_flat.cc:302-305)
    if (queries.empty())
      return {kEillegalParamteters, "vector_with_ids is empty"};
    std::vector<float> x;
    std::vector<uint8_t> xb;
    std::vector<int64_t> ids;
    Status s = binary_ ? pack_bits(queries, dim_, xb, ids)
                       : pack(queries, dim_, x, ids);
    if (!s.ok()) return s;
    dg_filter df{};
    dg_filter* dfp = nullptr;
    if (!fs.empty()) {
      if (fs.size() == 1 && fs[0]->ToDeviceFilter(&df)) dfp = &df;
      else return {kEVectorNotSupport, "composite filters via reader"};
    }
    float r = metric_ == MetricType::kL2 ? radius : 1.0f - radius;
    std::vector<int64_t> lims(queries.size() + 1);
    int64_t* rids = nullptr;
    float* rdists = nullptr;
    // binary: the reference hands its float radius to faiss's int parameter
    // (vector_index_flat.cc:304-308), i.e. truncates; distances pass through
    dg_status st =
        binary_ ? dg_range_search_binary(idx_, (int64_t)queries.size(),
                                         xb.data(), (int32_t)radius,
                                         p.binary_ivf_flat_nprobe, dfp,
                                         lims.data(), &rids, &rdists)
                : dg_range_search(idx_, (int64_t)queries.size(), x.data(), r,
                                  dfp, lims.data(), &rids, &rdists);
    if (st != DG_OK) return from_dg(st);
    results.clear();
    results.resize(queries.size());
    for (size_t q = 0; q < queries.size(); q++) {
      for (int64_t i = lims[q]; i < lims[q + 1]; i++) {
        VectorWithDistance vd;
        vd.vector_with_id.id = rids[i];
        vd.vector_with_id.vector.dimension = dim_;
        vd.metric_type = metric_;
        vd.distance = (metric_ == MetricType::kL2 ||
                       metric_ == MetricType::kHamming)
                          ? rdists[i]
                          : 1.0f - rdists[i];
        results[q].vector_with_distances.push_back(std::move(vd));
      }
    }
    dg_free(rids);
    dg_free(rdists);
    return Status::OK();
  }

 protected:
  static constexpr int64_t kNeedSaveCount = 10000;  // *_need_save_count
  static constexpr int64_t kMaxPointsPerCentroid = 256;  // faiss Clustering
  dg_index* idx_ = nullptr;
  dg_status create_st_ = DG_OK;
  MetricType metric_;
  int32_t dim_;
  bool binary_ = false;
  bool batching_ = false;  // set before the index is shared with the pool
  dg_batch_opts batch_opts_{};
  int32_t nlist_created_ = 0;  // nlist_org_ of the reference
  int64_t train_data_size_ = 0;
};

class GpuFlatIndex : public GpuIndexBase {
 public:
  GpuFlatIndex(MetricType m, int32_t d, int dev)
      : GpuIndexBase(DG_INDEX_FLAT, m, d, 0, dev) {}
  bool NeedTrain() override { return false; }
  // Flat has no NeedToRebuild trigger in the reference (base default false)
};

class GpuIvfFlatIndex : public GpuIndexBase {
 public:
  GpuIvfFlatIndex(MetricType m, int32_t d, int32_t nlist, int dev)
      : GpuIndexBase(DG_INDEX_IVF_FLAT, m, d, nlist, dev),
        nlist_org_(nlist) {}
  bool NeedTrain() override { return !IsTrained(); }
  bool NeedToRebuild() override {
    // restates vector_index_ivf_flat.cc:751-783: rebuild when the data has
    // outgrown the structure (degraded nlist, or the train sample is now
    // under half the data) past max_points_per_centroid * nlist
    dg_stats_out s{};
    if (dg_stats(idx_, &s) != DG_OK || !s.is_trained) return false;
    const int64_t nlist_now = s.nlist;  // degrades to 1 at small trains
    if (nlist_now == nlist_org_ && nlist_now == 1) return false;
    const bool grown = s.ntotal >= kMaxPointsPerCentroid * nlist_org_;
    if (nlist_now != nlist_org_ && nlist_now == 1 && grown) return true;
    if (nlist_now == nlist_org_ && nlist_now != 1 && grown)
      return train_data_size_ <= s.ntotal / 2;
    return false;
  }

 private:
  int64_t nlist_org_;
};

// IVF-Flat with the rows stored as IEEE halves (DG_STORAGE_F16).  The
// reference has no such index: no CPU node could read its snapshot as an
// IndexIVFFlat, so Save / Load speak the library's own container.
class GpuIvfFlatF16Index : public GpuIvfFlatIndex {
 public:
  GpuIvfFlatF16Index(MetricType m, int32_t d, int32_t nlist, int dev,
                     int32_t storage = DG_STORAGE_F16)
      : GpuIvfFlatIndex(m, d, nlist, dev), storage_(storage) {
    if (create_st_ == DG_OK) create_st_ = dg_set_storage(idx_, storage_);
  }
  Status Save(const std::string& path) override {
    return from_dg(dg_save(idx_, path.c_str()));
  }
  Status Load(const std::string& path) override {
    dg_index* ni = nullptr;
    dg_status st = dg_load(&ni, path.c_str(), -1);
    if (st != DG_OK) return from_dg(st);
    dg_stats_out got{};
    if (dg_stats(ni, &got) != DG_OK || got.kind != DG_INDEX_IVF_FLAT ||
        got.d != dim_ || got.metric != (int32_t)metric_ ||
        dg_get_storage(ni) != storage_) {
      dg_index_destroy(ni);
      return {kEInternal,
              "loaded index kind, dimension, metric or storage not match"};
    }
    dg_index_destroy(idx_);
    idx_ = ni;
    if (batching_) return EnableBatching(batch_opts_.max_batch,
                                         batch_opts_.max_wait_us);
    return Status::OK();
  }

 protected:
  int32_t storage_;
};

// IVF-Flat with one byte per component (DG_STORAGE_SQ8).  Train yields the
// per-dimension ranges next to the centroids (dg_train); Save / Load speak
// the library's own container, as for f16.
class GpuIvfFlatSq8Index : public GpuIvfFlatF16Index {
 public:
  GpuIvfFlatSq8Index(MetricType m, int32_t d, int32_t nlist, int dev)
      : GpuIvfFlatF16Index(m, d, nlist, dev, DG_STORAGE_SQ8) {}
};

class GpuBinaryFlatIndex : public GpuIndexBase {
 public:
  GpuBinaryFlatIndex(int32_t d, int dev)
      : GpuIndexBase(DG_INDEX_BINARY_FLAT, MetricType::kHamming, d, 0, dev) {}
  bool NeedTrain() override { return false; }
};

class GpuBinaryIvfFlatIndex : public GpuIndexBase {
 public:
  GpuBinaryIvfFlatIndex(int32_t d, int32_t nlist, int dev)
      : GpuIndexBase(DG_INDEX_BINARY_IVF_FLAT, MetricType::kHamming, d, nlist,
                     dev) {}
  bool NeedTrain() override { return !IsTrained(); }
};

class GpuIvfPqIndex : public GpuIndexBase {
 public:
  GpuIvfPqIndex(MetricType m, int32_t d, int32_t nlist, int32_t pq_m,
                int dev, int32_t pq_nbits = 8)
      : GpuIndexBase(DG_INDEX_IVF_PQ, m, d, nlist, dev, pq_m, pq_nbits) {}
  bool NeedTrain() override { return !IsTrained(); }
  bool NeedToRebuild() override {
    // vector_index_raw_ivf_pq.cc:518-526
    dg_stats_out s{};
    if (dg_stats(idx_, &s) != DG_OK || !s.is_trained) return false;
    return (s.ntotal / 2) >= train_data_size_;
  }
};

// VectorIndexHnsw (vector_index_hnsw.cc) over DG_INDEX_HNSW.  The overrides
// restate the reference's: Add is Upsert (:196), Delete of a missing id is
// EINTERNAL, the element count that IsExceedsMaxElements, NeedToRebuild and
// NeedToSave reason about is hnswlib's getCurrentElementCount, which counts
// deleted nodes (:531-610), Save / Load speak hnswlib's saveIndex container.
class GpuHnswIndex : public GpuIndexBase {
 public:
  GpuHnswIndex(MetricType m, int32_t d, int32_t nlinks, int32_t efc,
               int64_t max_elements, int dev)
      : GpuIndexBase(DG_INDEX_HNSW, m, d, 0, dev),
        max_elements_(max_elements), device_(dev) {
    if (create_st_ == DG_OK)
      create_st_ = dg_hnsw_configure(idx_, nlinks, efc, 100);
    if (create_st_ == DG_OK) dg_hnsw_max_elements(idx_, max_elements);
  }
  bool NeedTrain() override { return false; }
  Status Add(const std::vector<VectorWithId>& v) override {
    return Upsert(v);
  }
  Status Delete(const std::vector<int64_t>& ids) override {
    Status s = GpuIndexBase::Delete(ids);
    if (s.code == kEVectorInvalid) s.code = kEInternal;
    return s;
  }
  bool IsExceedsMaxElements(int64_t vector_size) override {
    dg_hnsw_info info{};
    if (dg_hnsw_get_info(idx_, &info) != DG_OK) return true;
    return info.n_nodes + vector_size > max_elements_;
  }
  bool NeedToRebuild() override {
    dg_hnsw_info info{};
    if (dg_hnsw_get_info(idx_, &info) != DG_OK) return false;
    if (info.n_nodes == 0 || info.n_deleted == 0) return false;
    return info.n_deleted > info.n_nodes / 2;
  }
  bool NeedToSave(int64_t last_save_log_behind) override {
    dg_hnsw_info info{};
    if (dg_hnsw_get_info(idx_, &info) != DG_OK || info.n_nodes == 0)
      return false;
    return last_save_log_behind > kNeedSaveCount;  // hnsw_need_save_count
  }
  bool SupportSave() override { return true; }
  Status Save(const std::string& path) override {
    return from_dg(dg_save_hnswlib(idx_, path.c_str()));
  }
  Status Load(const std::string& path) override {
    dg_hnsw_info info{};
    dg_status st = dg_hnsw_get_info(idx_, &info);
    if (st != DG_OK) return from_dg(st);
    dg_index* ni = nullptr;
    st = dg_load_hnswlib(&ni, path.c_str(), (int32_t)metric_, dim_, device_);
    if (st != DG_OK) return from_dg(st);
    (void)dg_hnsw_set_ef(ni, info.ef_search);
    // the limit is this index's parameter, as in the reference's loading
    // constructor, not the file's
    dg_hnsw_max_elements(ni, max_elements_);
    dg_index_destroy(idx_);
    idx_ = ni;
    if (batching_) return EnableBatching(batch_opts_.max_batch,
                                         batch_opts_.max_wait_us);
    return Status::OK();
  }
  Status Search(const std::vector<VectorWithId>& queries, uint32_t topk,
                const std::vector<std::shared_ptr<FilterFunctor>>& filters,
                bool reconstruct, const VectorSearchParameter& p,
                std::vector<VectorWithDistanceResult>& results) override {
    if (queries.empty())
      return {kEillegalParamteters, "vector_with_ids is empty"};
    if (topk == 0) return Status::OK();
    // vector_index_hnsw.cc:332
    if (p.hnsw_efsearch < 0 || p.hnsw_efsearch > 1024)
      return {kEillegalParamteters, "efsearch is illegal"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    Status s = pack(queries, dim_, x, ids);
    if (!s.ok()) return s;
    dg_filter df{};
    dg_filter* dfp = nullptr;
    if (!filters.empty()) {
      if (filters.size() == 1 && filters[0]->ToDeviceFilter(&df)) dfp = &df;
      else return {kEVectorNotSupport, "composite filters via reader fallback"};
    }
    std::vector<float> dist((size_t)queries.size() * topk);
    std::vector<int64_t> labels((size_t)queries.size() * topk, -1);
    dg_status st = dg_search_hnsw(idx_, (int64_t)queries.size(), x.data(),
                                  (int32_t)topk, p.hnsw_efsearch, dfp,
                                  dist.data(), labels.data());
    if (st != DG_OK) return from_dg(st);
    results.clear();
    results.resize(queries.size());
    std::vector<int64_t> found;
    for (size_t row = 0; row < queries.size(); row++)
      for (uint32_t i = 0; i < topk; i++) {
        const size_t pos = row * topk + i;
        if (labels[pos] < 0) continue;
        VectorWithDistance vd;
        vd.vector_with_id.id = labels[pos];
        vd.vector_with_id.vector.dimension = dim_;
        vd.metric_type = metric_;
        vd.distance =
            metric_ == MetricType::kL2 ? dist[pos] : 1.0f - dist[pos];
        results[row].vector_with_distances.push_back(std::move(vd));
        found.push_back(labels[pos]);
      }
    if (reconstruct && !found.empty()) {  // with_vector_data
      std::vector<float> rows(found.size() * (size_t)dim_);
      st = dg_reconstruct(idx_, (int64_t)found.size(), found.data(),
                          rows.data());
      if (st != DG_OK) return from_dg(st);
      size_t at = 0;
      for (auto& r : results)
        for (auto& vd : r.vector_with_distances) {
          vd.vector_with_id.vector.float_values.assign(
              rows.begin() + at * dim_, rows.begin() + (at + 1) * dim_);
          at++;
        }
    }
    return Status::OK();
  }

 private:
  int64_t max_elements_;
  int device_;  // as given to the factory (-1 = the current device)
};

// An index whose parameters the GPU library refuses (DG_ENOT_SUPPORT at
// create): every operation answers EVECTOR_NOT_SUPPORT, which is what sends
// the reader to its brute-force scan (SearchWithBruteForceFallback).
class GpuUnsupportedIndex : public VectorIndex {
 public:
  GpuUnsupportedIndex(MetricType m, int32_t d, std::string why)
      : metric_(m), dim_(d), why_(std::move(why)) {}
  int32_t GetDimension() override { return dim_; }
  MetricType GetMetricType() override { return metric_; }
  Status GetCount(int64_t& c) override { c = 0; return No(); }
  Status GetDeletedCount(int64_t& c) override { c = 0; return No(); }
  Status GetMemorySize(int64_t& b) override { b = 0; return No(); }
  bool IsExceedsMaxElements(int64_t) override { return false; }
  Status Add(const std::vector<VectorWithId>&) override { return No(); }
  Status Upsert(const std::vector<VectorWithId>&) override { return No(); }
  Status Delete(const std::vector<int64_t>&) override { return No(); }
  Status Train(const std::vector<VectorWithId>&) override { return No(); }
  Status Train(std::vector<float>&) override { return No(); }
  bool IsTrained() override { return false; }
  bool NeedTrain() override { return false; }
  bool NeedToRebuild() override { return false; }
  bool NeedToSave(int64_t) override { return false; }
  void LockWrite() override {}
  void UnlockWrite() override {}
  Status Save(const std::string&) override { return No(); }
  Status Load(const std::string&) override { return No(); }
  Status Search(const std::vector<VectorWithId>&, uint32_t,
                const std::vector<std::shared_ptr<FilterFunctor>>&, bool,
                const VectorSearchParameter&,
                std::vector<VectorWithDistanceResult>&) override {
    return No();
  }
  Status RangeSearch(const std::vector<VectorWithId>&, float,
                     const std::vector<std::shared_ptr<FilterFunctor>>&, bool,
                     const VectorSearchParameter&,
                     std::vector<VectorWithDistanceResult>&) override {
    return No();
  }

 private:
  Status No() const { return {kEVectorNotSupport, why_}; }
  MetricType metric_;
  int32_t dim_;
  std::string why_;
};

// One index over several devices of this process (dg_sharded_*): the same
// VectorIndex surface, the same 1 - score flip and error mapping as
// GpuIndexBase.  Save / Load of a sharded index are not offered.
class GpuShardedIndex : public VectorIndex {
 public:
  GpuShardedIndex(dg_index_kind kind, MetricType metric, int32_t dim,
                  int32_t nlist, int32_t pq_m, int32_t pq_nbits,
                  const std::vector<int>& devices)
      : kind_(kind), metric_(metric), dim_(dim) {
    dg_index_desc desc{};
    desc.kind = (int32_t)kind;
    desc.metric = (int32_t)metric;
    desc.d = dim;
    desc.nlist = nlist;
    desc.pq_m = pq_m;
    desc.pq_nbits = pq_nbits;
    std::vector<int32_t> devs(devices.begin(), devices.end());
    create_st_ = dg_sharded_create(&sh_, &desc, (int32_t)devs.size(),
                                   devs.data());
    create_status_ = from_dg(create_st_);
  }
  ~GpuShardedIndex() override {
    if (sh_) dg_sharded_destroy(sh_);
  }
  const Status& CreateStatus() const { return create_status_; }

  int32_t GetDimension() override { return dim_; }
  MetricType GetMetricType() override { return metric_; }
  Status GetCount(int64_t& count) override {
    dg_stats_out s{};
    dg_status st = dg_sharded_stats(sh_, &s);
    count = s.ntotal;
    return from_dg(st);
  }
  Status GetDeletedCount(int64_t& deleted_count) override {
    dg_stats_out s{};
    dg_status st = dg_sharded_stats(sh_, &s);
    deleted_count = s.deleted_count;
    return from_dg(st);
  }
  Status GetMemorySize(int64_t& bytes) override {
    dg_stats_out s{};
    dg_status st = dg_sharded_stats(sh_, &s);
    bytes = s.device_bytes;
    return from_dg(st);
  }
  bool IsExceedsMaxElements(int64_t) override { return false; }
  Status Add(const std::vector<VectorWithId>& v) override {
    if (v.empty()) return {kEillegalParamteters, "vector_with_ids is empty"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    Status s = pack(v, dim_, x, ids);
    if (!s.ok()) return s;
    return from_dg(
        dg_sharded_add(sh_, (int64_t)v.size(), ids.data(), x.data()));
  }
  Status Upsert(const std::vector<VectorWithId>& v) override {
    if (v.empty()) return {kEillegalParamteters, "vector_with_ids is empty"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    Status s = pack(v, dim_, x, ids);
    if (!s.ok()) return s;
    return from_dg(
        dg_sharded_upsert(sh_, (int64_t)v.size(), ids.data(), x.data()));
  }
  Status Delete(const std::vector<int64_t>& ids) override {
    if (ids.empty()) return {kEillegalParamteters, "empty ids"};
    return from_dg(dg_sharded_remove(sh_, (int64_t)ids.size(), ids.data()));
  }
  Status Train(const std::vector<VectorWithId>& v) override {
    if (v.empty()) return {kEillegalParamteters, "data size invalid"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    Status s = pack(v, dim_, x, ids);
    if (!s.ok()) return s;
    return from_dg(dg_sharded_train(sh_, (int64_t)v.size(), x.data()));
  }
  Status Train(std::vector<float>& train_datas) override {
    size_t data_size = train_datas.size() / dim_;
    if (data_size == 0)
      return {kEillegalParamteters, "data size invalid"};
    if (train_datas.size() % dim_ != 0)
      return {kEillegalParamteters, "dimension not match"};
    return from_dg(
        dg_sharded_train(sh_, (int64_t)data_size, train_datas.data()));
  }
  bool IsTrained() override {
    dg_stats_out s{};
    return dg_sharded_stats(sh_, &s) == DG_OK && s.is_trained;
  }
  bool NeedTrain() override {
    return kind_ != DG_INDEX_FLAT && !IsTrained();
  }
  bool NeedToRebuild() override { return false; }
  bool NeedToSave(int64_t) override { return false; }  // no Save
  bool SupportSave() override { return false; }
  // mutation and search of a sharded index lock inside the handle
  void LockWrite() override {}
  void UnlockWrite() override {}
  Status Save(const std::string&) override {
    return {kEVectorNotSupport, "save of a sharded index is not offered"};
  }
  Status Load(const std::string&) override {
    return {kEVectorNotSupport, "load of a sharded index is not offered"};
  }

  Status Search(const std::vector<VectorWithId>& queries, uint32_t topk,
                const std::vector<std::shared_ptr<FilterFunctor>>& filters,
                bool, const VectorSearchParameter& p,
                std::vector<VectorWithDistanceResult>& results) override {
    if (queries.empty())
      return {kEillegalParamteters, "vector_with_ids is empty"};
    if (topk == 0) return Status::OK();
    std::vector<float> x;
    std::vector<int64_t> ids;
    Status s = pack(queries, dim_, x, ids);
    if (!s.ok()) return s;
    dg_filter df{};
    dg_filter* dfp = nullptr;
    if (!filters.empty()) {
      if (filters.size() == 1 && filters[0]->ToDeviceFilter(&df))
        dfp = &df;
      else
        return {kEVectorNotSupport, "composite filters via reader fallback"};
    }
    std::vector<float> dist((size_t)queries.size() * topk);
    std::vector<int64_t> labels((size_t)queries.size() * topk, -1);
    dg_status st = dg_sharded_search(
        sh_, (int64_t)queries.size(), x.data(), (int32_t)topk,
        kind_ == DG_INDEX_IVF_PQ ? p.ivf_pq_nprobe : p.ivf_flat_nprobe, dfp,
        dist.data(), labels.data());
    if (st != DG_OK) return from_dg(st);
    results.clear();
    results.resize(queries.size());
    for (size_t row = 0; row < queries.size(); row++) {
      for (uint32_t i = 0; i < topk; i++) {
        size_t pos = row * topk + i;
        if (labels[pos] < 0) continue;  // padding skipped, utils.cc:622-624
        VectorWithDistance vd;
        vd.vector_with_id.id = labels[pos];
        vd.vector_with_id.vector.dimension = dim_;
        vd.metric_type = metric_;
        vd.distance =
            metric_ == MetricType::kL2 ? dist[pos] : 1.0f - dist[pos];
        results[row].vector_with_distances.push_back(std::move(vd));
      }
    }
    return Status::OK();
  }

  Status RangeSearch(const std::vector<VectorWithId>& queries, float radius,
                     const std::vector<std::shared_ptr<FilterFunctor>>& fs,
                     bool, const VectorSearchParameter&,
                     std::vector<VectorWithDistanceResult>& results) override {
    if (queries.empty())
      return {kEillegalParamteters, "vector_with_ids is empty"};
    std::vector<float> x;
    std::vector<int64_t> ids;
    Status s = pack(queries, dim_, x, ids);
    if (!s.ok()) return s;
    dg_filter df{};
    dg_filter* dfp = nullptr;
    if (!fs.empty()) {
      if (fs.size() == 1 && fs[0]->ToDeviceFilter(&df)) dfp = &df;
      else return {kEVectorNotSupport, "composite filters via reader"};
    }
    float r = metric_ == MetricType::kL2 ? radius : 1.0f - radius;
    std::vector<int64_t> lims(queries.size() + 1);
    int64_t* rids = nullptr;
    float* rdists = nullptr;
    dg_status st =
        dg_sharded_range_search(sh_, (int64_t)queries.size(), x.data(), r,
                                dfp, lims.data(), &rids, &rdists);
    if (st != DG_OK) return from_dg(st);
    results.clear();
    results.resize(queries.size());
    for (size_t q = 0; q < queries.size(); q++) {
      for (int64_t i = lims[q]; i < lims[q + 1]; i++) {
        VectorWithDistance vd;
        vd.vector_with_id.id = rids[i];
        vd.vector_with_id.vector.dimension = dim_;
        vd.metric_type = metric_;
        vd.distance =
            metric_ == MetricType::kL2 ? rdists[i] : 1.0f - rdists[i];
        results[q].vector_with_distances.push_back(std::move(vd));
      }
    }
    dg_free(rids);
    dg_free(rdists);
    return Status::OK();
  }

 private:
  dg_sharded* sh_ = nullptr;
  dg_status create_st_ = DG_OK;
  Status create_status_;
  dg_index_kind kind_;
  MetricType metric_;
  int32_t dim_;
};

std::unique_ptr<VectorIndex> new_sharded(dg_index_kind kind, MetricType metric,
                                         int32_t dim, int32_t nlist,
                                         int32_t pq_m, int32_t pq_nbits,
                                         const std::vector<int>& devices) {
  auto p = std::make_unique<GpuShardedIndex>(kind, metric, dim, nlist, pq_m,
                                             pq_nbits, devices);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

}  // namespace


// ---- reader brute-force fallback (vector_reader.cc:1873-2048) ----
namespace {
struct HeapEntry {  // DistanceResult analog (vector_reader.cc:1845-1858)
  float distance;
  VectorWithDistance vd;
  bool operator<(const HeapEntry& o) const { return distance < o.distance; }
};
}  // namespace

Status BruteForceSearch(MetricType metric, int32_t dimension,
                        const RowIterator& next,
                        const std::vector<VectorWithId>& queries,
                        uint32_t topk,
                        const std::vector<std::shared_ptr<FilterFunctor>>& f,
                        const VectorSearchParameter& p,
                        std::vector<VectorWithDistanceResult>& results,
                        int64_t batch_count) {
  if (dimension <= 0) return {kEVectorInvalid, "dimension invalid"};
  std::vector<std::priority_queue<HeapEntry>> tops(queries.size());
  std::vector<VectorWithId> batch;
  batch.reserve(batch_count);
  auto flush = [&]() -> Status {
    if (batch.empty()) return Status::OK();
    // throwaway per-batch Flat index (vector_reader.cc:1939-1942)
    auto flat = NewFlatIndex(metric, dimension);
    if (!flat) return {kEInternal, "flat index create failed"};
    Status s = flat->Add(batch);
    if (!s.ok()) return s;
    std::vector<VectorWithDistanceResult> rb;
    s = flat->Search(queries, topk, f, false, p, rb);
    if (!s.ok()) return s;
    for (size_t i = 0; i < rb.size(); i++) {
      auto& top = tops[i];
      for (auto& vd : rb[i].vector_with_distances) {
        if (top.size() < topk) {
          top.push({vd.distance, vd});
        } else if (top.top().distance > vd.distance) {
          top.pop();
          top.push({vd.distance, vd});
        }
      }
    }
    batch.clear();
    return Status::OK();
  };
  VectorWithId row;
  while (next(&row)) {
    batch.push_back(std::move(row));
    if ((int64_t)batch.size() == batch_count) {
      Status s = flush();
      if (!s.ok()) return s;
    }
  }
  Status s = flush();
  if (!s.ok()) return s;
  // ascending by distance (deque emplace_front, vector_reader.cc:2032-2044)
  results.clear();
  results.resize(queries.size());
  for (size_t i = 0; i < tops.size(); i++) {
    auto& top = tops[i];
    std::vector<VectorWithDistance> tmp;
    while (!top.empty()) {
      tmp.push_back(top.top().vd);
      top.pop();
    }
    results[i].vector_with_distances.assign(tmp.rbegin(), tmp.rend());
  }
  return Status::OK();
}

Status SearchWithBruteForceFallback(
    VectorIndex* index, const std::function<RowIterator()>& scan_factory,
    const std::vector<VectorWithId>& queries, uint32_t topk,
    const std::vector<std::shared_ptr<FilterFunctor>>& f,
    const VectorSearchParameter& p,
    std::vector<VectorWithDistanceResult>& results) {
  Status s = index->Search(queries, topk, f, false, p, results);
  if (s.code == kEVectorNotSupport) {
    // the reader's fallback trigger (vector_reader.cc:1828-1831)
    return BruteForceSearch(index->GetMetricType(), index->GetDimension(),
                            scan_factory(), queries, topk, f, p, results);
  }
  return s;
}

std::unique_ptr<VectorIndex> NewFlatIndex(MetricType metric, int32_t dim,
                                          int device) {
  auto p = std::make_unique<GpuFlatIndex>(metric, dim, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewIvfFlatIndex(MetricType metric, int32_t dim,
                                             int32_t ncentroids, int device) {
  auto p = std::make_unique<GpuIvfFlatIndex>(metric, dim, ncentroids, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewIvfFlatIndexF16(MetricType metric, int32_t dim,
                                                int32_t ncentroids,
                                                int device) {
  auto p =
      std::make_unique<GpuIvfFlatF16Index>(metric, dim, ncentroids, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewIvfFlatIndexSq8(MetricType metric, int32_t dim,
                                                int32_t ncentroids,
                                                int device) {
  auto p =
      std::make_unique<GpuIvfFlatSq8Index>(metric, dim, ncentroids, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewIvfPqIndex(MetricType metric, int32_t dim,
                                           int32_t ncentroids,
                                           int32_t nsubvector, int device) {
  auto p = std::make_unique<GpuIvfPqIndex>(metric, dim, ncentroids,
                                           nsubvector, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewIvfPqIndex(MetricType metric, int32_t dim,
                                           int32_t ncentroids,
                                           int32_t nsubvector,
                                           int32_t nbits_per_idx,
                                           int device) {
  // vector_index_ivf_pq.cc:64-66
  const int32_t nbits = (nbits_per_idx % 64) > 0 ? nbits_per_idx % 64 : 8;
  auto p = std::make_unique<GpuIvfPqIndex>(metric, dim, ncentroids,
                                           nsubvector, device, nbits);
  Status s = p->CreateStatus();
  if (s.code == kEVectorNotSupport)
    return std::make_unique<GpuUnsupportedIndex>(metric, dim, s.msg);
  if (!s.ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewHnswIndex(MetricType metric, int32_t dim,
                                          int32_t nlinks,
                                          int32_t efconstruction,
                                          int64_t max_elements, int device) {
  auto p = std::make_unique<GpuHnswIndex>(metric, dim, nlinks, efconstruction,
                                          max_elements, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewBinaryFlatIndex(int32_t dim, int device) {
  auto p = std::make_unique<GpuBinaryFlatIndex>(dim, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

std::unique_ptr<VectorIndex> NewBinaryIvfFlatIndex(int32_t dim,
                                                   int32_t ncentroids,
                                                   int device) {
  auto p = std::make_unique<GpuBinaryIvfFlatIndex>(dim, ncentroids, device);
  if (!p->CreateStatus().ok()) return nullptr;
  return p;
}

Status EnableBatching(VectorIndex* index, int32_t max_batch,
                      int32_t max_wait_us) {
  auto* g = dynamic_cast<GpuIndexBase*>(index);
  if (!g) return {kEVectorNotSupport, "not a GPU index"};
  return g->EnableBatching(max_batch, max_wait_us);
}

Status DisableBatching(VectorIndex* index) {
  auto* g = dynamic_cast<GpuIndexBase*>(index);
  if (!g) return {kEVectorNotSupport, "not a GPU index"};
  return g->DisableBatching();
}

std::unique_ptr<VectorIndex> NewShardedFlatIndex(MetricType metric,
                                                 int32_t dim,
                                                 std::vector<int> devices) {
  return new_sharded(DG_INDEX_FLAT, metric, dim, 0, 0, 0, devices);
}

std::unique_ptr<VectorIndex> NewShardedIvfFlatIndex(MetricType metric,
                                                    int32_t dim,
                                                    int32_t ncentroids,
                                                    std::vector<int> devices) {
  return new_sharded(DG_INDEX_IVF_FLAT, metric, dim, ncentroids, 0, 0,
                     devices);
}

std::unique_ptr<VectorIndex> NewShardedIvfPqIndex(MetricType metric,
                                                  int32_t dim,
                                                  int32_t ncentroids,
                                                  int32_t nsubvector,
                                                  int32_t nbits_per_idx,
                                                  std::vector<int> devices) {
  const int32_t nbits = (nbits_per_idx % 64) > 0 ? nbits_per_idx % 64 : 8;
  return new_sharded(DG_INDEX_IVF_PQ, metric, dim, ncentroids, nsubvector,
                     nbits, devices);
}

}  // namespace dingogpu

// 2-shard Flat indexes on device 0 through VectorIndex::Search.  The rows
// are the unit vectors e_0 .. e_5 scaled by (id + 1), so every distance is
// exact in float32 and the expected lists are known: checks the order, the
// 1 - score flip (IP) and that pads are skipped (k above the row count),
// then Delete / Upsert routing and the not-supported Save / Load.
extern "C" int dg_mirror_selftest_sharded(void) {
  using namespace dingogpu;
  if (dg_device_count() == 0) return 1;
  const int32_t d = 8, n = 6;
  std::vector<VectorWithId> rows(n);
  for (int i = 0; i < n; i++) {
    rows[i].id = 100 + i;
    rows[i].vector.dimension = d;
    rows[i].vector.float_values.assign(d, 0.f);
    rows[i].vector.float_values[i] = (float)(i + 1);
  }
  VectorWithId q;  // e_2 * 3: the row of id 102 itself
  q.vector.dimension = d;
  q.vector.float_values.assign(d, 0.f);
  q.vector.float_values[2] = 3.f;
  VectorSearchParameter p;
  std::vector<VectorWithDistanceResult> res;
  for (MetricType m : {MetricType::kL2, MetricType::kInnerProduct}) {
    auto idx = NewShardedFlatIndex(m, d, {0, 0});
    if (!idx) return 10;
    if (!idx->Add(rows).ok()) return 11;
    int64_t cnt = 0;
    if (!idx->GetCount(cnt).ok() || cnt != n) return 12;
    // k = 10 > 6 rows: four pads per query, all skipped
    if (!idx->Search({q}, 10, {}, false, p, res).ok()) return 13;
    if (res.size() != 1 || (int)res[0].vector_with_distances.size() != n)
      return 14;
    const auto& top = res[0].vector_with_distances;
    if (top[0].vector_with_id.id != 102) return 15;
    if (m == MetricType::kL2) {
      // |3 e_2 - (i+1) e_i|^2 = 9 + (i+1)^2 for i != 2, 0 for i = 2
      if (top[0].distance != 0.f) return 16;
      if (top[1].vector_with_id.id != 100 || top[1].distance != 10.f)
        return 17;
      if (top[5].vector_with_id.id != 105 || top[5].distance != 45.f)
        return 18;
    } else {
      // scores: 9 for id 102 and 0 for the rest; dingo reports 1 - score
      if (top[0].distance != 1.f - 9.f) return 19;
      for (int i = 1; i < n; i++)
        if (top[i].distance != 1.f) return 20;
    }
    for (int i = 1; i < n; i++)
      if (top[i - 1].distance > top[i].distance) return 21;
    if (!idx->Delete({102}).ok()) return 22;
    if (idx->Delete({102}).code != kEVectorInvalid) return 23;
    if (idx->Add({rows[0]}).code != kEVectorIdDuplicated) return 24;
    if (!idx->Search({q}, 1, {}, false, p, res).ok()) return 25;
    if (res[0].vector_with_distances.size() != 1 ||
        res[0].vector_with_distances[0].vector_with_id.id == 102)
      return 26;
    VectorWithId moved = rows[5];  // id 105 moves onto the query
    moved.vector.float_values = q.vector.float_values;
    if (!idx->Upsert({moved}).ok()) return 27;
    if (!idx->Search({q}, 1, {}, false, p, res).ok()) return 28;
    if (res[0].vector_with_distances[0].vector_with_id.id != 105) return 29;
    if (idx->Save("/nonexistent").code != kEVectorNotSupport ||
        idx->Load("/nonexistent").code != kEVectorNotSupport)
      return 30;
  }
  if (NewShardedFlatIndex(MetricType::kL2, d, {}) != nullptr) return 31;
  return 0;
}

// ---------------- self-test (GPU) ----------------
extern "C" int dg_mirror_selftest(void) {
  using namespace dingogpu;
#define DG_ST(x) fprintf(stderr, "[selftest] %s\n", x)
  DG_ST("flat loop");
  const int32_t d = 64, n = 500;
  for (MetricType m :
       {MetricType::kL2, MetricType::kInnerProduct, MetricType::kCosine}) {
    auto idx = NewFlatIndex(m, d);
    if (!idx) return 1;
    std::vector<VectorWithId> batch(n);
    uint32_t s = 12345;
    for (int i = 0; i < n; i++) {
      batch[i].id = i * 7 + 3;
      batch[i].vector.dimension = d;
      batch[i].vector.float_values.resize(d);
      for (int j = 0; j < d; j++) {
        s = s * 1664525u + 1013904223u;
        batch[i].vector.float_values[j] = (s >> 8) * (1.0f / 16777216.0f);
      }
    }
    if (!idx->Add(batch).ok()) return 2;
    std::vector<VectorWithDistanceResult> res;
    VectorSearchParameter p;
    if (!idx->Search(batch, 3, {}, false, p, res).ok()) return 3;
    if (res.size() != (size_t)n) return 4;
    for (int i = 0; i < n; i++) {
      if (res[i].vector_with_distances.empty()) return 5;
      // self-top-1 (test_vector_index_recall_flat.cc:170-236) holds for L2
      // and cosine; NOT for raw inner product (the max-IP neighbor of x
      // need not be x itself)
      if (m != MetricType::kInnerProduct &&
          res[i].vector_with_distances[0].vector_with_id.id != batch[i].id)
        return 6;
      float dist = res[i].vector_with_distances[0].distance;
      // L2 self-dist 0; cosine reported as 1 - score -> 0 for self
      if (m == MetricType::kL2 && std::fabs(dist) > 1e-3f) return 7;
      if (m == MetricType::kCosine && std::fabs(dist) > 1e-3f) return 8;
    }
    // range filter: restrict to ids < 100
    std::vector<std::shared_ptr<FilterFunctor>> f{
        std::make_shared<RangeFilterFunctor>(0, 100)};
    std::vector<VectorWithDistanceResult> res2;
    if (!idx->Search({batch[0]}, 5, f, false, p, res2).ok()) return 9;
    for (auto& vd : res2[0].vector_with_distances)
      if (vd.vector_with_id.id >= 100) return 10;
  }

  DG_ST("ivf lifecycle");
  // ---- IVF lifecycle through the mirror (Train/Add/Search/RangeSearch/
  // Upsert/Delete/Save/Load), L2 ----
  {
    const int32_t d2 = 32, n2 = 2000;
    auto ivf = NewIvfFlatIndex(MetricType::kL2, d2, 16);
    if (!ivf) return 20;
    std::vector<VectorWithId> batch(n2);
    uint32_t s = 99;
    for (int i = 0; i < n2; i++) {
      batch[i].id = i;
      batch[i].vector.dimension = d2;
      batch[i].vector.float_values.resize(d2);
      for (int j = 0; j < d2; j++) {
        s = s * 1664525u + 1013904223u;
        batch[i].vector.float_values[j] = (s >> 8) * (1.0f / 16777216.0f);
      }
    }
    if (ivf->IsTrained()) return 21;           // NeedTrain before Train
    if (!ivf->NeedTrain()) return 22;
    // untrained Search: blank results, OK (ivf_flat.cc:223-227)
    std::vector<VectorWithDistanceResult> r0;
    VectorSearchParameter p;
    p.ivf_flat_nprobe = 16;
    if (!ivf->Search({batch[0]}, 3, {}, false, p, r0).ok()) return 23;
    if (!r0[0].vector_with_distances.empty()) return 24;
    if (!ivf->Train(batch).ok()) return 25;
    if (!ivf->IsTrained()) return 26;
    if (!ivf->Add(batch).ok()) return 27;
    int64_t cnt = 0;
    ivf->GetCount(cnt);
    if (cnt != n2) return 28;
    std::vector<VectorWithDistanceResult> r1;
    if (!ivf->Search({batch[7]}, 3, {}, false, p, r1).ok()) return 29;
    if (r1[0].vector_with_distances.empty() ||
        r1[0].vector_with_distances[0].vector_with_id.id != 7)
      return 30;
    DG_ST("range search");
    // range search around the self-distance
    std::vector<VectorWithDistanceResult> r2;
    if (!ivf->RangeSearch({batch[7]}, 0.5f, {}, false, p, r2).ok())
      return 31;
    bool has_self = false;
    for (auto& vd : r2[0].vector_with_distances)
      if (vd.vector_with_id.id == 7) has_self = true;
    if (!has_self) return 32;
    DG_ST("delete+upsert");
    // delete + upsert
    if (!ivf->Delete({7}).ok()) return 33;
    int64_t delc = -1;
    if (!ivf->GetDeletedCount(delc).ok() || delc != 1) return 61;
    std::vector<VectorWithDistanceResult> r3;
    ivf->Search({batch[7]}, 1, {}, false, p, r3);
    if (!r3[0].vector_with_distances.empty() &&
        r3[0].vector_with_distances[0].vector_with_id.id == 7)
      return 34;
    if (!ivf->Upsert({batch[7]}).ok()) return 35;
    std::vector<VectorWithDistanceResult> r4;
    ivf->Search({batch[7]}, 1, {}, false, p, r4);
    if (r4[0].vector_with_distances.empty() ||
        r4[0].vector_with_distances[0].vector_with_id.id != 7)
      return 36;
    DG_ST("save/load");
    // save / load round trip
    const char* path = "/tmp/dg_mirror_selftest.dgi";
    if (!ivf->Save(path).ok()) return 37;
    if (!ivf->Load(path).ok()) return 38;
    std::vector<VectorWithDistanceResult> r5;
    ivf->Search({batch[7]}, 1, {}, false, p, r5);
    if (r5[0].vector_with_distances.empty() ||
        r5[0].vector_with_distances[0].vector_with_id.id != 7)
      return 39;
    DG_ST("dim mismatch");
    // dimension mismatch rejected (CheckVectorDimension semantics)
    VectorWithId bad;
    bad.id = 999999;
    bad.vector.dimension = d2 / 2;
    bad.vector.float_values.resize(d2 / 2);
    if (ivf->Add({bad}).ok()) return 40;

    DG_ST("lifecycle virtuals");
    // ---- wrapper-lifecycle virtuals (§8b must-implement set) ----
    if (!ivf->SupportSave()) return 41;
    if (ivf->IsExceedsMaxElements(1 << 20)) return 42;  // always false
    int64_t delc2 = -1;  // faiss-file load dropped the tombstones
    if (!ivf->GetDeletedCount(delc2).ok() || delc2 != 0) return 43;
    if (ivf->NeedToSave(100)) return 44;      // behind <= need_save_count
    if (!ivf->NeedToSave(20000)) return 45;   // behind > 10000
    if (ivf->NeedToRebuild()) return 46;      // ntotal < 256 * nlist
    ivf->LockWrite();   // exclusive fork-save window lock
    ivf->UnlockWrite();
    DG_ST("raw-float train");
    // raw-float Train(std::vector<float>&) on a fresh index
    {
      auto ivf2 = NewIvfFlatIndex(MetricType::kL2, d2, 4);
      if (!ivf2) return 47;
      std::vector<float> tdata;
      tdata.reserve((size_t)n2 * d2);
      for (auto& vw : batch)
        tdata.insert(tdata.end(), vw.vector.float_values.begin(),
                     vw.vector.float_values.end());
      std::vector<float> badsize(tdata.begin(), tdata.begin() + d2 / 2);
      if (ivf2->Train(badsize).ok()) return 48;  // size % dim != 0 rejected
      if (!ivf2->Train(tdata).ok()) return 49;
      if (!ivf2->IsTrained()) return 50;
    }
    DG_ST("concrete filter");
    // ConcreteFilterFunctor (IDSelectorBatch semantics) incl. Build hook
    {
      std::vector<int64_t> want{3, 9, 15};
      auto cf = std::make_shared<ConcreteFilterFunctor>(want);
      std::vector<int64_t> idmap;
      cf->Build(idmap);  // reference default no-op hook, callable
      if (!cf->Check(9) || cf->Check(10)) return 51;
      std::vector<std::shared_ptr<FilterFunctor>> fs{cf};
      std::vector<VectorWithDistanceResult> r6;
      if (!ivf->Search({batch[3]}, 3, fs, false, p, r6).ok()) return 52;
      if (r6[0].vector_with_distances.empty()) return 53;
      for (auto& vd : r6[0].vector_with_distances) {
        int64_t id = vd.vector_with_id.id;
        if (id != 3 && id != 9 && id != 15) return 54;
      }
      // negated form excludes them
      auto nf = std::make_shared<ConcreteFilterFunctor>(want, true);
      std::vector<std::shared_ptr<FilterFunctor>> fs2{nf};
      std::vector<VectorWithDistanceResult> r7;
      if (!ivf->Search({batch[3]}, 5, fs2, false, p, r7).ok()) return 55;
      for (auto& vd : r7[0].vector_with_distances) {
        int64_t id = vd.vector_with_id.id;
        if (id == 3 || id == 9 || id == 15) return 56;
      }
    }
  }

  // ---- reader brute-force path + EVECTOR_NOT_SUPPORT fallback round trip
  // (vector_reader.cc:1873-2048, :1828-1831) ----
  DG_ST("brute force");
  {
    const int32_t d3 = 24;
    const int64_t n3 = 5000;  // > 2 batches of 2048
    std::vector<VectorWithId> rows(n3);
    uint32_t s = 777;
    for (int64_t i = 0; i < n3; i++) {
      rows[i].id = i * 2 + 1;
      rows[i].vector.dimension = d3;
      rows[i].vector.float_values.resize(d3);
      for (int j = 0; j < d3; j++) {
        s = s * 1664525u + 1013904223u;
        rows[i].vector.float_values[j] = (s >> 8) * (1.0f / 16777216.0f);
      }
    }
    std::vector<VectorWithId> queries(rows.begin(), rows.begin() + 4);
    auto make_scan = [&]() -> RowIterator {
      auto pos = std::make_shared<int64_t>(0);
      return [&rows, pos](VectorWithId* out) {
        if (*pos >= (int64_t)rows.size()) return false;
        *out = rows[(*pos)++];
        return true;
      };
    };
    VectorSearchParameter p3;
    // ground truth: one persistent Flat index over all rows
    auto all = NewFlatIndex(MetricType::kL2, d3);
    if (!all) return 70;
    if (!all->Add(rows).ok()) return 71;
    std::vector<VectorWithDistanceResult> want;
    if (!all->Search(queries, 7, {}, false, p3, want).ok()) return 72;
    // KV-scan brute force (2048-row batches + heap merge) must agree
    std::vector<VectorWithDistanceResult> got;
    if (!BruteForceSearch(MetricType::kL2, d3, make_scan(), queries, 7, {},
                          p3, got).ok())
      return 73;
    if (got.size() != want.size()) return 74;
    for (size_t i = 0; i < got.size(); i++) {
      auto& g = got[i].vector_with_distances;
      auto& w = want[i].vector_with_distances;
      if (g.size() != w.size()) return 75;
      for (size_t j = 0; j < g.size(); j++) {
        if (g[j].vector_with_id.id != w[j].vector_with_id.id) return 76;
        if (std::fabs(g[j].distance - w[j].distance) > 1e-4f) return 77;
      }
    }
    // NOT_SUPPORT fallback round trip: an index that rejects the request
    // must transparently drop to the brute-force scan
    class NotSupportIndex : public GpuFlatIndex {
     public:
      NotSupportIndex(MetricType m, int32_t d) : GpuFlatIndex(m, d, -1) {}
      Status Search(const std::vector<VectorWithId>&, uint32_t,
                    const std::vector<std::shared_ptr<FilterFunctor>>&,
                    bool, const VectorSearchParameter&,
                    std::vector<VectorWithDistanceResult>&) override {
        return {kEVectorNotSupport, "not support"};
      }
    };
    NotSupportIndex ns(MetricType::kL2, d3);
    std::vector<VectorWithDistanceResult> got2;
    if (!SearchWithBruteForceFallback(&ns, make_scan, queries, 7, {}, p3,
                                      got2).ok())
      return 78;
    if (got2.size() != want.size()) return 79;
    for (size_t i = 0; i < got2.size(); i++)
      if (got2[i].vector_with_distances.size() !=
              want[i].vector_with_distances.size() ||
          got2[i].vector_with_distances[0].vector_with_id.id !=
              want[i].vector_with_distances[0].vector_with_id.id)
        return 80;
  }
  DG_ST("done");
  return 0;
}

// ---------------- self-test, binary indexes (GPU) ----------------
extern "C" int dg_mirror_selftest_binary(void) {
  using namespace dingogpu;
  const int32_t d = 200, n = 1500;  // 25 bytes: word + tail per row
  std::vector<VectorWithId> batch(n);
  uint32_t s = 4242;
  for (int i = 0; i < n; i++) {
    batch[i].id = i * 3 + 1;
    batch[i].vector.dimension = d;
    batch[i].vector.value_type = ValueType::kUint8;
    batch[i].vector.binary_values.resize(d / 8);
    for (int j = 0; j < d / 8; j++) {
      s = s * 1664525u + 1013904223u;
      batch[i].vector.binary_values[j] = (uint8_t)(s >> 24);
    }
  }
  auto hamming = [&](const VectorWithId& a, const VectorWithId& b) {
    int h = 0;
    for (int j = 0; j < d / 8; j++)
      h += __builtin_popcount(a.vector.binary_values[j] ^
                              b.vector.binary_values[j]);
    return h;
  };
  for (int kind = 0; kind < 2; kind++) {
    auto idx = kind == 0 ? NewBinaryFlatIndex(d) : NewBinaryIvfFlatIndex(d, 8);
    if (!idx) return 100 + kind;
    if (idx->GetMetricType() != MetricType::kHamming) return 102;
    VectorSearchParameter p;
    p.binary_ivf_flat_nprobe = 8;
    if (kind == 1) {
      if (idx->IsTrained() || !idx->NeedTrain()) return 103;
      if (!idx->Train(batch).ok()) return 104;
      if (!idx->IsTrained()) return 105;
    }
    if (!idx->Add(batch).ok()) return 106;
    int64_t cnt = 0;
    if (!idx->GetCount(cnt).ok() || cnt != n) return 107;
    std::vector<VectorWithId> queries(batch.begin(), batch.begin() + 40);
    std::vector<VectorWithDistanceResult> res;
    if (!idx->Search(queries, 4, {}, false, p, res).ok()) return 108;
    if (res.size() != queries.size()) return 109;
    for (size_t i = 0; i < queries.size(); i++) {
      auto& r = res[i].vector_with_distances;
      if (r.size() != 4) return 110;
      // self top-1 at distance 0 (random 200-bit rows are distinct)
      if (r[0].vector_with_id.id != queries[i].id || r[0].distance != 0.f)
        return 111;
      // Hamming pass-through: the reported distance is the integer
      // distance to the returned row, ascending, not flipped
      for (size_t j = 0; j < r.size(); j++) {
        const int64_t row = (r[j].vector_with_id.id - 1) / 3;
        if (row < 0 || row >= n) return 112;
        if (r[j].distance != (float)hamming(queries[i], batch[row]))
          return 113;
        if (j && r[j].distance < r[j - 1].distance) return 114;
        if (r[j].metric_type != MetricType::kHamming) return 115;
      }
    }
    // wrong byte count is rejected
    VectorWithId bad = batch[0];
    bad.id = 999999;
    bad.vector.binary_values.resize(d / 8 - 1);
    if (idx->Add({bad}).code != kEVectorInvalid) return 116;
    if (idx->Search({bad}, 1, {}, false, p, res).code != kEVectorInvalid)
      return 117;
    // delete then search: the row is gone
    if (!idx->Delete({batch[5].id}).ok()) return 118;
    if (!idx->Search({batch[5]}, 1, {}, false, p, res).ok()) return 119;
    if (!res[0].vector_with_distances.empty() &&
        res[0].vector_with_distances[0].vector_with_id.id == batch[5].id)
      return 120;
    if (!idx->Upsert({batch[5]}).ok()) return 121;
    if (!idx->Search({batch[5]}, 1, {}, false, p, res).ok()) return 122;
    if (res[0].vector_with_distances.empty() ||
        res[0].vector_with_distances[0].vector_with_id.id != batch[5].id)
      return 123;
    // range search against the hamming lambda: every row strictly below
    // the radius, ascending, with its distance passed through
    int64_t live = 0;
    if (!idx->GetCount(live).ok() || live != n) return 124;
    std::vector<VectorWithDistanceResult> rr;
    const float radius = 85.9f;  // truncates to 85
    if (!idx->RangeSearch(queries, radius, {}, false, p, rr).ok()) return 124;
    if (rr.size() != queries.size()) return 124;
    for (size_t i = 0; i < queries.size(); i++) {
      auto& r = rr[i].vector_with_distances;
      size_t want = 0;
      for (int j = 0; j < n; j++)
        if (hamming(queries[i], batch[j]) < 85) want++;
      if (r.size() != want || want == 0) return 124;
      for (size_t j = 0; j < r.size(); j++) {
        const int64_t row = (r[j].vector_with_id.id - 1) / 3;
        if (row < 0 || row >= n) return 124;
        if (r[j].distance != (float)hamming(queries[i], batch[row]) ||
            r[j].distance >= 85.f)
          return 124;
        if (j && r[j].distance < r[j - 1].distance) return 124;
        if (r[j].metric_type != MetricType::kHamming) return 124;
      }
    }
    // Save -> Load into a fresh index -> the same top-4
    if (!idx->SupportSave()) return 125;
    const std::string path = "/tmp/dg_mirror_selftest_binary." +
                             std::to_string((long)getpid()) + "." +
                             std::to_string(kind) + ".idx";
    std::vector<VectorWithDistanceResult> before, after;
    if (!idx->Search(queries, 4, {}, false, p, before).ok()) return 125;
    if (!idx->Save(path).ok()) return 125;
    auto fresh =
        kind == 0 ? NewBinaryFlatIndex(d) : NewBinaryIvfFlatIndex(d, 8);
    Status ls = fresh ? fresh->Load(path) : Status{kEInternal, "create"};
    // a file of the other kind, or of another dimension, is refused
    auto other =
        kind == 0 ? NewBinaryIvfFlatIndex(d, 8) : NewBinaryFlatIndex(d);
    auto wide = kind == 0 ? NewBinaryFlatIndex(d + 8)
                          : NewBinaryIvfFlatIndex(d + 8, 8);
    bool refused = other && wide && !other->Load(path).ok() &&
                   !wide->Load(path).ok();
    if (kind == 1) {  // an IVF file of another nlist
      auto more = NewBinaryIvfFlatIndex(d, 16);
      refused = refused && more && !more->Load(path).ok();
    }
    remove(path.c_str());
    if (!ls.ok() || !refused) return 126;
    int64_t cnt2 = 0;
    if (!fresh->GetCount(cnt2).ok() || cnt2 != n || !fresh->IsTrained())
      return 126;
    if (!fresh->Search(queries, 4, {}, false, p, after).ok()) return 126;
    if (after.size() != before.size()) return 126;
    for (size_t i = 0; i < before.size(); i++) {
      auto& a = before[i].vector_with_distances;
      auto& b = after[i].vector_with_distances;
      if (a.size() != b.size()) return 126;
      // equal distances; ids equal wherever the distance is not tied (the
      // row order inside a list may differ after a reload)
      for (size_t j = 0; j < a.size(); j++) {
        if (a[j].distance != b[j].distance) return 126;
        const bool tied =
            (j && a[j - 1].distance == a[j].distance) ||
            (j + 1 < a.size() && a[j + 1].distance == a[j].distance) ||
            j + 1 == a.size();
        if (!tied && a[j].vector_with_id.id != b[j].vector_with_id.id)
          return 126;
      }
    }
  }
  return 0;
}

// ---------------- self-test: IVF-PQ at nbits_per_idx = 4 (GPU) -------------
extern "C" int dg_mirror_selftest_pq4(void) {
  using namespace dingogpu;
  if (dg_device_count() == 0) return 1;
  const int d = 16, m = 8, nlist = 4, n = 1000;
  std::vector<VectorWithId> batch(n);
  uint32_t s = 777;
  for (int i = 0; i < n; i++) {
    batch[i].id = i * 5 + 2;
    batch[i].vector.dimension = d;
    batch[i].vector.float_values.resize(d);
    for (int j = 0; j < d; j++) {
      s = s * 1664525u + 1013904223u;
      batch[i].vector.float_values[j] = (float)(s >> 8) / 16777216.0f;
    }
  }
  VectorSearchParameter p;
  p.ivf_flat_nprobe = nlist;
  p.ivf_pq_nprobe = nlist;
  // 64 + 4 normalises to 4 like the reference's % 64
  auto idx = NewIvfPqIndex(MetricType::kL2, d, nlist, m, 64 + 4, -1);
  if (!idx) return 200;
  if (idx->IsTrained() || !idx->NeedTrain()) return 201;
  if (!idx->Train(batch).ok()) return 202;
  if (!idx->IsTrained()) return 203;
  if (!idx->Add(batch).ok()) return 204;
  int64_t cnt = 0;
  if (!idx->GetCount(cnt).ok() || cnt != n) return 205;
  std::vector<VectorWithId> queries(batch.begin(), batch.begin() + 40);
  std::vector<VectorWithDistanceResult> before, after;
  if (!idx->Search(queries, 4, {}, false, p, before).ok()) return 206;
  if (before.size() != queries.size()) return 207;
  for (size_t i = 0; i < queries.size(); i++) {
    auto& r = before[i].vector_with_distances;
    if (r.size() != 4) return 208;
    // a row's own 16-codeword reconstruction is far nearer than any other
    // row of 1000 uniform points in 16 dimensions
    if (r[0].vector_with_id.id != queries[i].id) return 209;
    for (size_t j = 1; j < r.size(); j++)
      if (r[j].distance < r[j - 1].distance) return 210;
  }
  // Save (faiss IwPQ, nbits = 4, packed codes) -> Load -> the same top-4
  const std::string path = "/tmp/dg_mirror_selftest_pq4." +
                           std::to_string((long)getpid()) + ".idx";
  if (!idx->SupportSave() || !idx->Save(path).ok()) return 211;
  auto fresh = NewIvfPqIndex(MetricType::kL2, d, nlist, m, 4, -1);
  Status ls = fresh ? fresh->Load(path) : Status{kEInternal, "create"};
  remove(path.c_str());
  if (!ls.ok()) return 212;
  int64_t cnt2 = 0;
  if (!fresh->GetCount(cnt2).ok() || cnt2 != n || !fresh->IsTrained())
    return 213;
  if (!fresh->Search(queries, 4, {}, false, p, after).ok()) return 214;
  if (after.size() != before.size()) return 215;
  for (size_t i = 0; i < before.size(); i++) {
    auto& a = before[i].vector_with_distances;
    auto& b = after[i].vector_with_distances;
    if (a.size() != b.size()) return 216;
    // equal distances; ids equal wherever the distance is not tied (the
    // row order inside a list may differ after a reload)
    for (size_t j = 0; j < a.size(); j++) {
      if (a[j].distance != b[j].distance) return 217;
      const bool tied =
          (j && a[j - 1].distance == a[j].distance) ||
          (j + 1 < a.size() && a[j + 1].distance == a[j].distance) ||
          j + 1 == a.size();
      if (!tied && a[j].vector_with_id.id != b[j].vector_with_id.id)
        return 218;
    }
  }
  // nbits_per_idx = 0 takes the default 8 and creates a working index
  auto def8 = NewIvfPqIndex(MetricType::kL2, d, nlist, m, 0, -1);
  if (!def8 || !def8->Train(batch).ok()) return 219;
  // an unsupported width answers EVECTOR_NOT_SUPPORT and the reader's
  // brute-force scan serves the search
  auto odd = NewIvfPqIndex(MetricType::kL2, d, nlist, m, 5, -1);
  if (!odd) return 220;
  if (odd->Train(batch).code != kEVectorNotSupport) return 221;
  std::vector<VectorWithDistanceResult> bf;
  if (odd->Search(queries, 4, {}, false, p, bf).code != kEVectorNotSupport)
    return 222;
  auto factory = [&]() -> RowIterator {
    auto pos = std::make_shared<size_t>(0);
    return [&batch, pos](VectorWithId* out) {
      if (*pos >= batch.size()) return false;
      *out = batch[(*pos)++];
      return true;
    };
  };
  if (!SearchWithBruteForceFallback(odd.get(), factory, queries, 4, {}, p, bf)
           .ok())
    return 223;
  if (bf.size() != queries.size()) return 224;
  for (size_t i = 0; i < queries.size(); i++) {
    auto& r = bf[i].vector_with_distances;
    if (r.size() != 4 || r[0].vector_with_id.id != queries[i].id) return 225;
  }
  return 0;
}

// ---------------- self-test: search batching (GPU) ----------------
namespace {

// the reference pool's call shape: n_threads threads, one query per Search,
// released together; thread t takes queries t, t + n_threads, ...
int pool_search(dingogpu::VectorIndex* idx,
                const std::vector<dingogpu::VectorWithId>& queries,
                uint32_t topk,
                const std::vector<std::shared_ptr<dingogpu::FilterFunctor>>& f,
                const dingogpu::VectorSearchParameter& p, int n_threads,
                std::vector<dingogpu::VectorWithDistanceResult>* out) {
  using namespace dingogpu;
  out->assign(queries.size(), {});
  std::atomic<int> ready{0}, failed{0};
  std::vector<std::thread> th;
  for (int t = 0; t < n_threads; t++)
    th.emplace_back([&, t] {
      ready++;
      while (ready.load() < n_threads) std::this_thread::yield();
      for (size_t i = t; i < queries.size(); i += n_threads) {
        std::vector<VectorWithDistanceResult> r;
        if (!idx->Search({queries[i]}, topk, f, false, p, r).ok() ||
            r.size() != 1)
          failed++;
        else
          (*out)[i] = std::move(r[0]);
      }
    });
  for (auto& t : th) t.join();
  return failed.load();
}

// the comparison rule of batched against direct answers: the same ids,
// distances within rel (0 = equal)
bool same_answers(const std::vector<dingogpu::VectorWithDistanceResult>& a,
                  const std::vector<dingogpu::VectorWithDistanceResult>& b,
                  float rel) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++) {
    auto& x = a[i].vector_with_distances;
    auto& y = b[i].vector_with_distances;
    if (x.size() != y.size()) return false;
    for (size_t j = 0; j < x.size(); j++) {
      if (x[j].vector_with_id.id != y[j].vector_with_id.id) return false;
      if (std::fabs(x[j].distance - y[j].distance) >
          rel * std::fabs(y[j].distance))
        return false;
    }
  }
  return true;
}

}  // namespace

extern "C" int dg_mirror_selftest_f16(void) {
  using namespace dingogpu;
  if (dg_device_count() == 0) return 1;
  const int d = 20, nlist = 4, n = 600;
  std::vector<VectorWithId> batch(n);
  uint32_t s = 4242;
  for (int i = 0; i < n; i++) {
    batch[i].id = i * 3 + 1;
    batch[i].vector.dimension = d;
    batch[i].vector.float_values.resize(d);
    for (int j = 0; j < d; j++) {
      s = s * 1664525u + 1013904223u;
      // multiples of 1/64 in [0, 4): exact in half, so a row is its own
      // stored form and its self distance is exactly 0
      batch[i].vector.float_values[j] = (float)(s >> 24) / 64.0f;
    }
  }
  VectorSearchParameter p;
  p.ivf_flat_nprobe = nlist;
  auto idx = NewIvfFlatIndexF16(MetricType::kL2, d, nlist, -1);
  if (!idx) return 300;
  if (idx->IsTrained() || !idx->NeedTrain()) return 301;
  if (!idx->Train(batch).ok()) return 302;
  if (!idx->Add(batch).ok()) return 303;
  int64_t cnt = 0;
  if (!idx->GetCount(cnt).ok() || cnt != n) return 304;
  std::vector<VectorWithId> queries(batch.begin(), batch.begin() + 40);
  std::vector<VectorWithDistanceResult> before, after;
  if (!idx->Search(queries, 4, {}, false, p, before).ok()) return 305;
  if (before.size() != queries.size()) return 306;
  for (size_t i = 0; i < queries.size(); i++) {
    auto& r = before[i].vector_with_distances;
    if (r.size() != 4) return 307;
    if (r[0].distance != 0.0f) return 308;
    for (size_t j = 1; j < r.size(); j++)
      if (r[j].distance < r[j - 1].distance) return 309;
  }
  // a component no half can hold fails the whole Add
  std::vector<VectorWithId> bad(batch.begin(), batch.begin() + 2);
  bad[0].id = 100001;
  bad[1].id = 100002;
  bad[1].vector.float_values[3] = 70000.0f;
  if (idx->Add(bad).code != kEillegalParamteters) return 310;
  if (!idx->GetCount(cnt).ok() || cnt != n) return 311;
  // Save (the library's container) -> Load -> the same answers
  const std::string path = "/tmp/dg_mirror_selftest_f16." +
                           std::to_string((long)getpid()) + ".dgi";
  if (!idx->SupportSave() || !idx->Save(path).ok()) return 312;
  auto fresh = NewIvfFlatIndexF16(MetricType::kL2, d, nlist, -1);
  Status ls = fresh ? fresh->Load(path) : Status{kEInternal, "create"};
  remove(path.c_str());
  if (!ls.ok()) return 313;
  int64_t cnt2 = 0;
  if (!fresh->GetCount(cnt2).ok() || cnt2 != n || !fresh->IsTrained())
    return 314;
  if (!fresh->Search(queries, 4, {}, false, p, after).ok()) return 315;
  if (after.size() != before.size()) return 316;
  for (size_t i = 0; i < before.size(); i++) {
    auto& a = before[i].vector_with_distances;
    auto& b = after[i].vector_with_distances;
    if (a.size() != b.size()) return 317;
    for (size_t j = 0; j < a.size(); j++) {
      if (a[j].distance != b[j].distance) return 318;
      const bool tied =
          (j && a[j - 1].distance == a[j].distance) ||
          (j + 1 < a.size() && a[j + 1].distance == a[j].distance) ||
          j + 1 == a.size();
      if (!tied && a[j].vector_with_id.id != b[j].vector_with_id.id)
        return 319;
    }
  }
  return 0;
}

extern "C" int dg_mirror_selftest_sq8(void) {
  using namespace dingogpu;
  if (dg_device_count() == 0) return 1;
  const int d = 20, nlist = 4, n = 600;
  std::vector<VectorWithId> batch(n);
  uint32_t s = 777;
  for (int i = 0; i < n; i++) {
    batch[i].id = i * 3 + 1;
    batch[i].vector.dimension = d;
    batch[i].vector.float_values.resize(d);
    for (int j = 0; j < d; j++) {
      s = s * 1664525u + 1013904223u;
      batch[i].vector.float_values[j] = (float)(s >> 20) / 1024.0f;  // [0, 4)
    }
  }
  VectorSearchParameter p;
  p.ivf_flat_nprobe = nlist;
  auto idx = NewIvfFlatIndexSq8(MetricType::kL2, d, nlist, -1);
  if (!idx) return 400;
  if (idx->IsTrained() || !idx->NeedTrain()) return 401;
  // no ranges yet: Add is refused
  if (idx->Add(batch).ok()) return 402;
  if (!idx->Train(batch).ok()) return 403;  // centroids and ranges
  if (!idx->IsTrained()) return 404;
  if (!idx->Add(batch).ok()) return 405;
  int64_t cnt = 0;
  if (!idx->GetCount(cnt).ok() || cnt != n) return 406;
  std::vector<VectorWithId> queries(batch.begin(), batch.begin() + 40);
  std::vector<VectorWithDistanceResult> before, after;
  if (!idx->Search(queries, 4, {}, false, p, before).ok()) return 407;
  if (before.size() != queries.size()) return 408;
  // a row lies within half a step (range / 510, range < 4) of its stored
  // form in every dimension: its self distance is below d * (4 / 510)^2,
  // three orders of magnitude under the distance to another row
  const float self_max = d * (4.0f / 510.0f) * (4.0f / 510.0f) * 1.01f;
  for (size_t i = 0; i < queries.size(); i++) {
    auto& r = before[i].vector_with_distances;
    if (r.size() != 4) return 409;
    if (r[0].vector_with_id.id != queries[i].id) return 410;
    if (!(r[0].distance <= self_max)) return 411;
    for (size_t j = 1; j < r.size(); j++)
      if (r[j].distance < r[j - 1].distance) return 412;
  }
  // a NaN component fails the whole Add
  std::vector<VectorWithId> bad(batch.begin(), batch.begin() + 2);
  bad[0].id = 100001;
  bad[1].id = 100002;
  bad[1].vector.float_values[3] = std::nanf("");
  if (idx->Add(bad).code != kEillegalParamteters) return 413;
  if (!idx->GetCount(cnt).ok() || cnt != n) return 414;
  // Save (the library's container) -> Load -> the same answers
  const std::string path = "/tmp/dg_mirror_selftest_sq8." +
                           std::to_string((long)getpid()) + ".dgi";
  if (!idx->SupportSave() || !idx->Save(path).ok()) return 415;
  auto fresh = NewIvfFlatIndexSq8(MetricType::kL2, d, nlist, -1);
  Status ls = fresh ? fresh->Load(path) : Status{kEInternal, "create"};
  // an f16 index refuses the SQ8 file
  auto other = NewIvfFlatIndexF16(MetricType::kL2, d, nlist, -1);
  const bool refused = other && !other->Load(path).ok();
  remove(path.c_str());
  if (!ls.ok()) return 416;
  if (!refused) return 417;
  int64_t cnt2 = 0;
  if (!fresh->GetCount(cnt2).ok() || cnt2 != n || !fresh->IsTrained())
    return 418;
  if (!fresh->Search(queries, 4, {}, false, p, after).ok()) return 419;
  if (after.size() != before.size()) return 420;
  for (size_t i = 0; i < before.size(); i++) {
    auto& a = before[i].vector_with_distances;
    auto& b = after[i].vector_with_distances;
    if (a.size() != b.size()) return 421;
    for (size_t j = 0; j < a.size(); j++) {
      if (a[j].distance != b[j].distance) return 422;
      const bool tied =
          (j && a[j - 1].distance == a[j].distance) ||
          (j + 1 < a.size() && a[j + 1].distance == a[j].distance) ||
          j + 1 == a.size();
      if (!tied && a[j].vector_with_id.id != b[j].vector_with_id.id)
        return 423;
    }
  }
  return 0;
}

extern "C" int dg_mirror_selftest_hnsw(void) {
  using namespace dingogpu;
  if (dg_device_count() == 0) return 1;
  const int d = 12, n = 500;
  std::vector<VectorWithId> batch(n);
  uint32_t s = 4242;
  for (int i = 0; i < n; i++) {
    batch[i].id = i * 2 + 5;
    batch[i].vector.dimension = d;
    batch[i].vector.float_values.resize(d);
    for (int j = 0; j < d; j++) {
      s = s * 1664525u + 1013904223u;
      batch[i].vector.float_values[j] = (float)((int)(s >> 24) % 9 - 4);
    }
    batch[i].vector.float_values[i % d] += 0.25f * (float)(i / d + 1);
  }
  VectorSearchParameter p;
  p.hnsw_efsearch = 64;
  for (MetricType metric : {MetricType::kL2, MetricType::kInnerProduct}) {
    auto idx = NewHnswIndex(metric, d, 8, 100, 1000, -1);
    if (!idx) return 500;
    if (!idx->IsTrained() || idx->NeedTrain() || !idx->SupportSave())
      return 501;
    if (idx->NeedToSave(20000)) return 502;  // empty
    if (!idx->Add(batch).ok()) return 503;
    if (!idx->Add({batch[3]}).ok()) return 504;  // Add is Upsert
    int64_t cnt = 0, del = 0;
    if (!idx->GetCount(cnt).ok() || cnt != n) return 505;
    if (!idx->GetDeletedCount(del).ok() || del != 1) return 506;
    if (idx->IsExceedsMaxElements(499) || !idx->IsExceedsMaxElements(500))
      return 507;  // 501 nodes of 1000
    if (!idx->NeedToSave(20000) || idx->NeedToSave(10)) return 508;
    std::vector<VectorWithId> queries(batch.begin(), batch.begin() + 30);
    std::vector<VectorWithDistanceResult> before, after, filtered;
    if (!idx->Search(queries, 4, {}, true, p, before).ok()) return 509;
    if (before.size() != queries.size()) return 510;
    if (metric == MetricType::kL2)
      for (size_t i = 0; i < queries.size(); i++) {
        auto& r = before[i].vector_with_distances;
        if (r.size() != 4) return 511;
        if (r[0].vector_with_id.id != queries[i].id || r[0].distance != 0.f)
          return 512;
        if (r[0].vector_with_id.vector.float_values !=
            queries[i].vector.float_values)
          return 513;  // with_vector_data
        for (size_t j = 1; j < r.size(); j++)
          if (r[j].distance < r[j - 1].distance) return 514;
      }
    else  // the reported distance is 1 - score, ascending
      for (size_t i = 0; i < queries.size(); i++) {
        auto& r = before[i].vector_with_distances;
        if (r.size() != 4) return 515;
        for (size_t j = 0; j < r.size(); j++) {
          float dot = 0.f;
          for (int t = 0; t < d; t++)
            dot += queries[i].vector.float_values[t] *
                   r[j].vector_with_id.vector.float_values[t];
          if (std::fabs(r[j].distance - (1.0f - dot)) >
              1e-4f * (1.0f + std::fabs(dot)))
            return 516;
          if (j && r[j].distance < r[j - 1].distance) return 517;
        }
      }
    // a range filter holds for every answer
    auto f = std::make_shared<RangeFilterFunctor>(100, 300);
    if (!idx->Search(queries, 4, {f}, false, p, filtered).ok()) return 518;
    for (auto& r : filtered) {
      if (r.vector_with_distances.size() != 4) return 519;
      for (auto& vd : r.vector_with_distances)
        if (vd.vector_with_id.id < 100 || vd.vector_with_id.id >= 300)
          return 520;
    }
    VectorSearchParameter bad = p;
    bad.hnsw_efsearch = 1025;
    if (idx->Search(queries, 4, {}, false, bad, after).code !=
        kEillegalParamteters)
      return 521;
    std::vector<VectorWithDistanceResult> rr;
    if (idx->RangeSearch(queries, 1.0f, {}, false, p, rr).code !=
        kEVectorNotSupport)
      return 522;
    // Delete: a missing id is EINTERNAL and removes nothing
    if (idx->Delete({batch[0].id, 999999}).code != kEInternal) return 523;
    if (!idx->GetCount(cnt).ok() || cnt != n) return 524;
    if (!idx->Delete({batch[0].id}).ok()) return 525;
    std::vector<VectorWithDistanceResult> gone;
    if (!idx->Search({batch[0]}, 4, {}, false, p, gone).ok()) return 526;
    for (auto& vd : gone[0].vector_with_distances)
      if (vd.vector_with_id.id == batch[0].id) return 527;
    if (idx->NeedToRebuild()) return 528;  // 2 deleted of 501
    // Save (hnswlib container) -> Load -> the same answers
    if (!idx->Search(queries, 4, {}, false, p, before).ok()) return 529;
    const std::string path = "/tmp/dg_mirror_selftest_hnsw." +
                             std::to_string((long)getpid()) + ".bin";
    if (!idx->Save(path).ok()) return 530;
    auto fresh = NewHnswIndex(metric, d, 8, 100, 1000, -1);
    Status ls = fresh ? fresh->Load(path) : Status{kEInternal, "create"};
    auto wrong = NewHnswIndex(metric, d + 1, 8, 100, 1000, -1);
    const bool refused = wrong && !wrong->Load(path).ok();
    remove(path.c_str());
    if (!ls.ok()) return 531;
    if (!refused) return 532;
    if (!fresh->GetCount(cnt).ok() || cnt != n - 1) return 533;
    if (!fresh->GetDeletedCount(del).ok() || del != 2) return 534;
    if (!fresh->Search(queries, 4, {}, false, p, after).ok()) return 535;
    if (after.size() != before.size()) return 536;
    for (size_t i = 0; i < before.size(); i++) {
      auto& a = before[i].vector_with_distances;
      auto& b = after[i].vector_with_distances;
      if (a.size() != b.size()) return 537;
      for (size_t j = 0; j < a.size(); j++)
        if (a[j].distance != b[j].distance ||
            a[j].vector_with_id.id != b[j].vector_with_id.id)
          return 538;
    }
    // more than half deleted: rebuild
    std::vector<int64_t> half;
    for (int i = 1; i <= 260; i++) half.push_back(batch[i].id);
    if (!fresh->Delete(half).ok()) return 539;
    if (!fresh->NeedToRebuild()) return 540;
  }
  // a geometry the library refuses
  if (NewHnswIndex(MetricType::kL2, d, 1, 100, 1000, -1)) return 541;
  return 0;
}

extern "C" int dg_mirror_selftest_batched(void) {
  using namespace dingogpu;
  if (dg_device_count() == 0) return 1;
  const int32_t d = 64, n = 4000, nq = 48, threads = 16;
  std::vector<VectorWithId> batch(n);
  uint32_t s = 2024;
  for (int i = 0; i < n; i++) {
    batch[i].id = i * 2 + 1;
    batch[i].vector.dimension = d;
    batch[i].vector.float_values.resize(d);
    for (int j = 0; j < d; j++) {
      s = s * 1664525u + 1013904223u;
      batch[i].vector.float_values[j] = (s >> 8) * (1.0f / 16777216.0f);
    }
  }
  // queries: rows with a little deterministic noise
  std::vector<VectorWithId> queries(batch.begin(), batch.begin() + nq);
  for (auto& q : queries)
    for (auto& v : q.vector.float_values) {
      s = s * 1664525u + 1013904223u;
      v += ((s >> 8) * (1.0f / 16777216.0f) - 0.5f) * 0.1f;
    }
  const std::vector<std::shared_ptr<FilterFunctor>> none;
  const std::vector<std::shared_ptr<FilterFunctor>> lower_half{
      std::make_shared<RangeFilterFunctor>(0, n)};  // ids 1, 3, .. < n
  std::vector<VectorWithDistanceResult> direct, direct_f, got;

  // ---- IVF-Flat L2, without and with the region-range filter ----
  {
    auto ivf = NewIvfFlatIndex(MetricType::kL2, d, 16);
    if (!ivf) return 300;
    VectorSearchParameter p;
    p.ivf_flat_nprobe = 8;
    if (!ivf->Train(batch).ok() || !ivf->Add(batch).ok()) return 301;
    // the same calls unbatched (batching is off until EnableBatching)
    if (pool_search(ivf.get(), queries, 5, none, p, 1, &direct)) return 302;
    if (pool_search(ivf.get(), queries, 5, lower_half, p, 1, &direct_f))
      return 303;
    for (auto& r : direct_f)
      for (auto& vd : r.vector_with_distances)
        if (vd.vector_with_id.id >= n) return 304;
    // a batch waits up to 1 ms for company here, so that batches form
    // whatever the scheduling
    if (!EnableBatching(ivf.get(), 16, 1000).ok()) return 305;
    if (pool_search(ivf.get(), queries, 5, none, p, threads, &got)) return 306;
    if (!same_answers(got, direct, 1e-4f)) return 307;
    if (pool_search(ivf.get(), queries, 5, lower_half, p, threads, &got))
      return 308;
    if (!same_answers(got, direct_f, 1e-4f)) return 309;
    dg_batch_stats bs{};
    auto* g = dynamic_cast<GpuIndexBase*>(ivf.get());
    if (!g || !g->BatchingStats(&bs).ok()) return 310;
    if (bs.calls != 2 * nq || bs.queries != 2 * nq || bs.bypassed != 0)
      return 311;
    if (bs.max_flush_queries < 2 || bs.flushes >= 2 * nq) return 312;
    // off again: Search is the plain path and answers the same
    if (!DisableBatching(ivf.get()).ok()) return 313;
    if (pool_search(ivf.get(), queries, 5, none, p, threads, &got)) return 314;
    if (!same_answers(got, direct, 1e-4f)) return 315;
    if (!g->BatchingStats(&bs).ok() || bs.calls != 2 * nq) return 316;
  }

  // ---- Flat inner product: the 1 - score flip survives batching ----
  {
    auto flat = NewFlatIndex(MetricType::kInnerProduct, d);
    if (!flat) return 320;
    VectorSearchParameter p;
    if (!flat->Add(batch).ok()) return 321;
    if (pool_search(flat.get(), queries, 5, none, p, 1, &direct)) return 322;
    if (!EnableBatching(flat.get()).ok()) return 323;  // defaults: 64, no wait
    if (pool_search(flat.get(), queries, 5, none, p, threads, &got))
      return 324;
    if (!same_answers(got, direct, 1e-4f)) return 325;
    for (int i = 0; i < nq; i++) {
      auto& r = got[i].vector_with_distances;
      if (r.size() != 5) return 326;
      for (auto& vd : r) {
        const auto& row = batch[(vd.vector_with_id.id - 1) / 2];
        double dot = 0;
        for (int j = 0; j < d; j++)
          dot += (double)queries[i].vector.float_values[j] *
                 row.vector.float_values[j];
        // reported = 1 - score (vector_index_utils.cc:634)
        if (std::fabs((double)vd.distance - (1.0 - dot)) >
            1e-4 * std::fabs(dot))
          return 327;
      }
    }
  }

  // ---- binary Flat: integer distances, equal outputs ----
  {
    const int32_t db = 256;
    std::vector<VectorWithId> rows(n);
    for (int i = 0; i < n; i++) {
      rows[i].id = i * 3 + 1;
      rows[i].vector.dimension = db;
      rows[i].vector.value_type = ValueType::kUint8;
      rows[i].vector.binary_values.resize(db / 8);
      for (auto& v : rows[i].vector.binary_values) {
        s = s * 1664525u + 1013904223u;
        v = (uint8_t)(s >> 24);
      }
    }
    std::vector<VectorWithId> bq(rows.begin(), rows.begin() + nq);
    for (auto& q : bq) q.vector.binary_values[3] ^= 0x5a;
    auto bin = NewBinaryFlatIndex(db);
    if (!bin) return 330;
    VectorSearchParameter p;
    if (!bin->Add(rows).ok()) return 331;
    if (pool_search(bin.get(), bq, 5, none, p, 1, &direct)) return 332;
    if (!EnableBatching(bin.get()).ok()) return 333;
    if (pool_search(bin.get(), bq, 5, none, p, threads, &got)) return 334;
    if (!same_answers(got, direct, 0.f)) return 335;
  }

  // an index that is not GPU-backed has nothing to batch
  auto odd = NewIvfPqIndex(MetricType::kL2, 16, 4, 8, 5, -1);
  if (!odd || EnableBatching(odd.get()).code != kEVectorNotSupport) return 340;
  return 0;
}

extern "C" double dg_bench_threads(dg_index* idx, int32_t threads,
                                   int32_t calls_per_thread, int32_t batched,
                                   const float* q, int64_t nq, int32_t k,
                                   int32_t nprobe) {
  if (!idx || !q || threads <= 0 || calls_per_thread <= 0 || nq <= 0 ||
      k <= 0)
    return -1.0;
  dg_stats_out so{};
  if (dg_stats(idx, &so) != DG_OK) return -1.0;
  const int32_t d = so.d;
  std::atomic<int> ready{0}, failed{0};
  std::chrono::steady_clock::time_point t0;
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++)
    th.emplace_back([&, t] {
      std::vector<float> dist(k);
      std::vector<int64_t> ids(k);
      auto call = [&](int c) {
        const float* x = q + (size_t)((t * calls_per_thread + c) % nq) * d;
        const dg_status st =
            batched ? dg_search_batched(idx, 1, x, k, nprobe, nullptr,
                                        dist.data(), ids.data())
                    : dg_search(idx, 1, x, k, nprobe, nullptr, dist.data(),
                                ids.data());
        if (st != DG_OK) failed++;
      };
      call(0);  // untimed: dg_search allocates this thread's staging
      ready++;
      while (ready.load() <= threads) std::this_thread::yield();
      for (int c = 0; c < calls_per_thread; c++) call(c);
    });
  while (ready.load() < threads) std::this_thread::yield();
  t0 = std::chrono::steady_clock::now();
  ready++;  // go
  for (auto& t : th) t.join();
  const double sec = std::chrono::duration<double>(
                         std::chrono::steady_clock::now() - t0).count();
  return failed.load() ? -2.0 : sec;
}
