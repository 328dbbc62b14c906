// dg_batch.cpp — dg_search_batched: concurrent small searches of one index
// coalesced into device batches (include/dingo_gpu.h, DESIGN.md "Search
// batching").  The queue logic is dg_batch_core.h; this file validates the
// call, builds the compatibility key, owns the device staging and runs the
// flush: one H2D copy, one search, two D2H copies, one synchronize.
#include <algorithm>
#include <cstring>
#include <string>

#include "dg_batch_core.h"
#include "dg_internal.h"

namespace {

constexpr int32_t kDefaultMaxBatch = 64;
constexpr int32_t kMaxMaxBatch = 1024;

struct DevGuard {
  int prev = -1;
  explicit DevGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (dev >= 0 && dev != prev) (void)hipSetDevice(dev);
  }
  ~DevGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace

// Device staging belongs to the batcher, not to the calling thread: the
// leader changes from flush to flush, and per-thread dg_dbuf staging would
// grow once per leader and invalidate every captured graph each time.  Plain
// hipMalloc here: no graph refers to these buffers (the graph path copies
// the queries into the index's own ws_gq first).
struct dg_batcher {
  dg_index* ix;
  size_t row_bytes;
  int32_t max_batch = 0;
  // touched by the flushing leader only (flushes are serialized)
  void* d_q = nullptr;
  float* d_dist = nullptr;
  int64_t* d_ids = nullptr;
  int32_t d_kcap = 0;
  std::mutex cfg_mu;  // enable / disable against each other
  dgb::Batcher core;

  explicit dg_batcher(dg_index* ix_)
      : ix(ix_),
        row_bytes(ix_->is_bin ? (size_t)ix_->d_user / 8
                              : (size_t)ix_->d_user * 4),
        core(dgb::Hooks{
            [this](size_t n) -> void* {
              DevGuard g(ix->device);
              void* p = nullptr;
              if (hipHostMalloc(&p, n, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                return nullptr;
              }
              return p;
            },
            [this](void* p) {
              DevGuard g(ix->device);
              (void)hipHostFree(p);
            },
            [this](const dgb::Flush& f, std::string* err) {
              return flush(f, err);
            }}) {}

  void free_device() {
    DevGuard g(ix->device);
    if (d_q) (void)hipFree(d_q);
    if (d_dist) (void)hipFree(d_dist);
    if (d_ids) (void)hipFree(d_ids);
    d_q = nullptr;
    d_dist = nullptr;
    d_ids = nullptr;
    d_kcap = 0;
  }

  // result slabs for k columns; the previous flush has synchronized, so
  // nothing on the stream still uses the old ones
  dg_status reserve_out(int32_t k) {
    if (k <= d_kcap) return DG_OK;
    if (d_dist) (void)hipFree(d_dist);
    if (d_ids) (void)hipFree(d_ids);
    d_dist = nullptr;
    d_ids = nullptr;
    d_kcap = 0;
    if (hipMalloc((void**)&d_dist, (size_t)max_batch * k * 4) != hipSuccess ||
        hipMalloc((void**)&d_ids, (size_t)max_batch * k * 8) != hipSuccess) {
      (void)hipGetLastError();
      dg_set_error("batch staging: hipMalloc for k=%d failed", k);
      return DG_ENOMEM;
    }
    d_kcap = k;
    return DG_OK;
  }

  dg_status flush_impl(const dgb::Flush& f) {
    DevGuard g(ix->device);
    dg_status st = reserve_out(f.k);
    if (st != DG_OK) return st;
    {
      // not inside a bypassed call's graph capture (dg_index::capture_mu)
      std::shared_lock<std::shared_mutex> cl(ix->capture_mu);
      DG_HIP_CHECK(hipMemcpyAsync(d_q, f.q, (size_t)f.nq * row_bytes,
                                  hipMemcpyHostToDevice, ix->stream));
    }
    dg_filter flt{};
    flt.kind = f.key.filter_kind;
    flt.negate = f.key.negate;
    flt.min_id = f.key.min_id;
    flt.max_id = f.key.max_id;
    st = dg_search_device_flush(
        ix, f.nq, d_q, f.k, f.key.nprobe,
        flt.kind == DG_FILTER_NONE ? nullptr : &flt, d_dist, d_ids,
        ix->is_bin);
    std::shared_lock<std::shared_mutex> cl(ix->capture_mu);
    if (st != DG_OK) {
      // leave nothing of this flush on the stream behind the next one
      (void)hipStreamSynchronize(ix->stream);
      return st;
    }
    DG_HIP_CHECK(hipMemcpyAsync(f.dist, d_dist, (size_t)f.nq * f.k * 4,
                                hipMemcpyDeviceToHost, ix->stream));
    DG_HIP_CHECK(hipMemcpyAsync(f.ids, d_ids, (size_t)f.nq * f.k * 8,
                                hipMemcpyDeviceToHost, ix->stream));
    DG_HIP_CHECK(hipStreamSynchronize(ix->stream));
    return DG_OK;
  }

  int flush(const dgb::Flush& f, std::string* err) {
    dg_status st = flush_impl(f);
    if (st != DG_OK) {
      // dg_last_error is thread-local: hand the text to the members
      char buf[1024];
      dg_last_error(buf, sizeof(buf));
      *err = buf;
    }
    return (int)st;
  }
};

void dg_batcher_destroy(dg_batcher* b) {
  if (!b) return;
  b->core.disable();
  b->free_device();
  delete b;
}

extern "C" dg_status dg_batching_enable(dg_index* ix,
                                        const dg_batch_opts* opts) {
  if (!ix) {
    dg_set_error("null index");
    return DG_EINVAL;
  }
  int32_t max_batch = opts ? opts->max_batch : 0;
  const int32_t max_wait_us = opts ? opts->max_wait_us : 0;
  if (max_batch == 0) max_batch = kDefaultMaxBatch;
  if (max_batch < 1 || max_batch > kMaxMaxBatch || max_wait_us < 0) {
    dg_set_error("dg_batching_enable: need 0 <= max_batch <= %d and "
                 "max_wait_us >= 0 (got %d, %d)", kMaxMaxBatch,
                 opts ? opts->max_batch : 0, max_wait_us);
    return DG_EINVAL;
  }
  dg_batcher* b = ix->batcher.load(std::memory_order_acquire);
  if (!b) {
    dg_batcher* nb = new dg_batcher(ix);
    if (ix->batcher.compare_exchange_strong(b, nb,
                                            std::memory_order_acq_rel))
      b = nb;
    else
      delete nb;  // another thread was first; b holds its batcher
  }
  std::lock_guard<std::mutex> lk(b->cfg_mu);
  b->core.disable();  // drained: no flush is using the device staging
  DevGuard g(ix->device);
  if (b->max_batch != max_batch) {
    b->free_device();
    if (hipMalloc(&b->d_q, (size_t)max_batch * b->row_bytes) != hipSuccess) {
      (void)hipGetLastError();
      b->max_batch = 0;
      dg_set_error("batch staging: hipMalloc failed");
      return DG_ENOMEM;
    }
    b->max_batch = max_batch;
  }
  dg_status st = b->reserve_out(dgb::Batcher::kInitialK);
  if (st != DG_OK) return st;
  if (!b->core.enable(max_batch, max_wait_us, b->row_bytes)) {
    dg_set_error("batch staging: pinned host allocation failed");
    return DG_ENOMEM;
  }
  return DG_OK;
}

extern "C" dg_status dg_batching_disable(dg_index* ix) {
  if (!ix) {
    dg_set_error("null index");
    return DG_EINVAL;
  }
  dg_batcher* b = ix->batcher.load(std::memory_order_acquire);
  if (!b) return DG_OK;
  std::lock_guard<std::mutex> lk(b->cfg_mu);
  b->core.disable();
  return DG_OK;
}

extern "C" dg_status dg_batching_stats(dg_index* ix, dg_batch_stats* out) {
  if (!ix || !out) {
    dg_set_error("null arg");
    return DG_EINVAL;
  }
  *out = {};
  dg_batcher* b = ix->batcher.load(std::memory_order_acquire);
  if (!b) return DG_OK;
  const dgb::Stats s = b->core.stats();
  out->calls = s.calls;
  out->queries = s.queries;
  out->flushes = s.flushes;
  out->max_flush_queries = s.max_flush_queries;
  out->bypassed = s.bypassed;
  return DG_OK;
}

static dg_status search_batched_impl(dg_index* ix, int64_t nq, const void* x,
                                     int32_t k, int32_t nprobe,
                                     const dg_filter* filter, float* out_dist,
                                     int64_t* out_ids, bool binary) {
  auto direct = [&]() {
    return binary ? dg_search_binary(ix, nq, (const uint8_t*)x, k, nprobe,
                                     filter, out_dist, out_ids)
                  : dg_search(ix, nq, (const float*)x, k, nprobe, filter,
                              out_dist, out_ids);
  };
  dg_batcher* b = ix ? ix->batcher.load(std::memory_order_acquire) : nullptr;
  if (!b) return direct();
  // Validation comes before the queue, so a bad call cannot fail a batch.
  // What dg_search rejects or answers without searching (argument errors,
  // k <= 0, k above the limit, the wrong entry-point family) goes to
  // dg_search itself: same status, same message, never a batch.
  if (!x || !out_dist || !out_ids || nq <= 0 || k <= 0 || k > 2048 ||
      ix->is_bin != binary)
    return direct();
  if (dg_kind_is_hnsw(ix->desc.kind)) {
    // one wave per query already: a graph search gains nothing from a merge
    (void)b->core.note_bypass(nq);
    return direct();
  }
  dgb::Key key;
  if (filter && filter->kind != DG_FILTER_NONE) {
    if (filter->kind != DG_FILTER_RANGE) {
      // id lists and bitmaps differ per call; merging them would need
      // per-query pass bitmaps in the scan
      (void)b->core.note_bypass(nq);
      return direct();
    }
    key.filter_kind = DG_FILTER_RANGE;
    key.negate = filter->negate;
    key.min_id = filter->min_id;
    key.max_id = filter->max_id;
  }
  if (!dg_kind_is_flat(ix->desc.kind)) {
    int32_t nlist;
    {
      std::shared_lock<std::shared_mutex> lk(ix->rw);  // train changes nlist
      nlist = ix->desc.nlist;
    }
    int32_t np = nprobe > 0 ? nprobe : 80;  // as search_core resolves it
    np = std::min(np, nlist);
    if (np < nlist && np > 2048) return direct();  // DG_ENOT_SUPPORT there
    key.nprobe = np;
  }
  std::string err;
  const int st = b->core.submit(x, nq, k, key, out_dist, out_ids, &err);
  if (st == dgb::kNotEnabled || st == dgb::kBypassed) return direct();
  if (st != DG_OK) dg_set_error("%s", err.c_str());
  return (dg_status)st;
}

extern "C" dg_status dg_search_batched(dg_index* ix, int64_t nq,
                                       const float* x, int32_t k,
                                       int32_t nprobe,
                                       const dg_filter* filter,
                                       float* out_dist, int64_t* out_ids) {
  return search_batched_impl(ix, nq, x, k, nprobe, filter, out_dist, out_ids,
                             false);
}

extern "C" dg_status dg_search_binary_batched(dg_index* ix, int64_t nq,
                                              const uint8_t* x, int32_t k,
                                              int32_t nprobe,
                                              const dg_filter* filter,
                                              float* out_dist,
                                              int64_t* out_ids) {
  return search_batched_impl(ix, nq, x, k, nprobe, filter, out_dist, out_ids,
                             true);
}
