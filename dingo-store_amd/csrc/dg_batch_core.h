// dg_batch_core.h — the queue logic of dg_search_batched, free of HIP.
//
// Concurrent callers that each bring a few queries are merged into one
// device batch.  There is no dispatcher thread: the caller that opens a
// batch leads it, the callers that join it follow.
//   - a call joins the open batch of its compatibility key (dgb::Key) if it
//     fits, otherwise it closes that batch and opens the next one; a call is
//     never split, and a call of max_batch queries or more is not batched
//   - every member copies its own query rows into the batch's staging slab
//   - batches flush one at a time in the order they were opened.  The leader
//     flushes once the previous flush has returned ("the device is free");
//     it then waits at most max_wait_us for the batch to fill
//   - the flush runs at the largest k of the members; every member copies
//     the first k_i columns of its own rows out of the result slabs
//   - a failed flush hands its status and message to each of its members
// The flush itself and the allocation of the (pinned) slabs are callables,
// so a CPU program can drive this file with a fake device
// (tests/host/batch_core_test.cpp).
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace dgb {

// What two calls must share to run as one search: the resolved nprobe and
// the filter (none, or an id range with equal bounds).
struct Key {
  int32_t nprobe = 0;
  int32_t filter_kind = 0;
  int32_t negate = 0;
  int64_t min_id = 0, max_id = 0;
  bool operator==(const Key& o) const {
    return nprobe == o.nprobe && filter_kind == o.filter_kind &&
           negate == o.negate && min_id == o.min_id && max_id == o.max_id;
  }
};

// One flush: nq query rows in q, results to dist/ids as [nq x k].
struct Flush {
  Key key;
  int64_t nq = 0;
  int32_t k = 0;
  const void* q = nullptr;
  float* dist = nullptr;
  int64_t* ids = nullptr;
};

struct Hooks {
  // slab memory (pinned host memory in the library); alloc may return null
  std::function<void*(size_t)> alloc;
  std::function<void(void*)> release;
  // 0 on success, else a status and its message
  std::function<int(const Flush&, std::string* err)> flush;
};

struct Stats {
  int64_t calls = 0, queries = 0, flushes = 0, max_flush_queries = 0,
          bypassed = 0;
};

// submit() answers besides a flush status (>= 0)
enum : int {
  kNotEnabled = -1,  // batching is off: the caller searches directly
  kBypassed = -2     // counted; the caller searches directly
};
constexpr int kNoMemory = 4;  // DG_ENOMEM

class Batcher {
 public:
  static constexpr int32_t kInitialK = 128;  // columns the result slabs start with

  explicit Batcher(Hooks hooks) : hooks_(std::move(hooks)) {}
  Batcher(const Batcher&) = delete;
  ~Batcher() {
    disable();
    std::lock_guard<std::mutex> lk(mu_);
    drop_pool();
  }

  // Drains, then (re)starts with these settings and zeroed statistics.
  // Two slabs are allocated here: one flushing, one filling.
  bool enable(int32_t max_batch, int32_t max_wait_us, size_t row_bytes) {
    std::unique_lock<std::mutex> lk(mu_);
    enabled_ = false;
    cv_.wait(lk, [&] { return inflight_ == 0; });
    if (max_batch != max_batch_ || row_bytes != row_bytes_) drop_pool();
    max_batch_ = max_batch;
    max_wait_us_ = max_wait_us;
    row_bytes_ = row_bytes;
    while (pool_.size() < 2) {
      Slab s;
      if (!new_slab(&s)) return false;
      pool_.push_back(s);
    }
    stats_ = Stats();
    enabled_ = true;
    return true;
  }

  // Later calls are not batched; returns once every batched call has left.
  void disable() {
    std::unique_lock<std::mutex> lk(mu_);
    enabled_ = false;
    cv_.wait(lk, [&] { return inflight_ == 0; });
  }

  bool enabled() {
    std::lock_guard<std::mutex> lk(mu_);
    return enabled_;
  }

  Stats stats() {
    std::lock_guard<std::mutex> lk(mu_);
    return stats_;
  }

  // A call the caller runs directly for a reason of its own (a filter that
  // cannot be merged).  False if batching is off.
  bool note_bypass(int64_t nq) {
    std::lock_guard<std::mutex> lk(mu_);
    if (!enabled_) return false;
    stats_.calls++;
    stats_.queries += nq;
    stats_.bypassed++;
    return true;
  }

  // Blocks until the caller's rows are in out_dist / out_ids ([nq x k]).
  // The arguments are valid (nq >= 1, k >= 1, non-null buffers).
  int submit(const void* x, int64_t nq, int32_t k, const Key& key,
             float* out_dist, int64_t* out_ids, std::string* err) {
    std::unique_lock<std::mutex> lk(mu_);
    if (!enabled_) return kNotEnabled;
    stats_.calls++;
    stats_.queries += nq;
    if (nq >= max_batch_) {
      stats_.bypassed++;
      return kBypassed;
    }
    std::shared_ptr<Batch> b;
    for (auto& c : queue_) {
      if (c->closed || !(c->key == key)) continue;
      if (c->nq + nq <= max_batch_) {
        b = c;
      } else {
        c->closed = true;  // the next call would overflow it
        cv_.notify_all();
      }
      break;  // a key has at most one open batch
    }
    const bool leader = !b;
    if (leader) {
      b = std::make_shared<Batch>();
      b->key = key;
      if (!pool_.empty()) {
        b->slab = pool_.back();
        pool_.pop_back();
      } else if (!new_slab(&b->slab)) {
        if (err) *err = "batch staging allocation failed";
        return kNoMemory;
      }
      queue_.push_back(b);
    }
    const int64_t row0 = b->nq;
    b->nq += nq;
    b->kmax = std::max(b->kmax, k);
    b->members++;
    b->copying++;
    inflight_++;
    if (b->nq == max_batch_) {
      b->closed = true;
      cv_.notify_all();
    }
    lk.unlock();
    memcpy((char*)b->slab.q + (size_t)row0 * row_bytes_, x,
           (size_t)nq * row_bytes_);
    lk.lock();
    if (--b->copying == 0) cv_.notify_all();

    if (leader) {
      // the device is free once the previous flush has returned and every
      // batch opened before this one has gone
      cv_.wait(lk, [&] { return !flushing_ && queue_.front() == b; });
      if (max_wait_us_ > 0 && !b->closed)
        cv_.wait_for(lk, std::chrono::microseconds(max_wait_us_),
                     [&] { return b->closed; });
      b->closed = true;
      cv_.wait(lk, [&] { return b->copying == 0; });
      queue_.pop_front();
      flushing_ = true;
      stats_.flushes++;
      stats_.max_flush_queries = std::max(stats_.max_flush_queries, b->nq);
      if (b->kmax > b->slab.kcap && !grow_slab(&b->slab, b->kmax)) {
        b->status = kNoMemory;
        b->err = "batch staging allocation failed";
      } else {
        lk.unlock();
        Flush f;
        f.key = b->key;
        f.nq = b->nq;
        f.k = b->kmax;
        f.q = b->slab.q;
        f.dist = b->slab.dist;
        f.ids = b->slab.ids;
        std::string msg;
        const int st = hooks_.flush(f, &msg);
        lk.lock();
        b->status = st;
        if (st != 0) b->err = std::move(msg);
      }
      flushing_ = false;
      b->done = true;
      cv_.notify_all();
    } else {
      cv_.wait(lk, [&] { return b->done; });
    }

    const int st = b->status;
    if (st != 0 && err) *err = b->err;
    lk.unlock();
    if (st == 0) {
      // top-k_i is the first k_i columns of top-kmax: results are best-first
      // under a total order
      const size_t km = (size_t)b->kmax;
      for (int64_t r = 0; r < nq; r++) {
        memcpy(out_dist + (size_t)r * k, b->slab.dist + (size_t)(row0 + r) * km,
               (size_t)k * sizeof(float));
        memcpy(out_ids + (size_t)r * k, b->slab.ids + (size_t)(row0 + r) * km,
               (size_t)k * sizeof(int64_t));
      }
    }
    lk.lock();
    if (--b->members == 0) pool_.push_back(b->slab);
    if (--inflight_ == 0) cv_.notify_all();
    return st;
  }

 private:
  struct Slab {
    void* q = nullptr;       // [max_batch x row_bytes]
    float* dist = nullptr;   // [max_batch x kcap]
    int64_t* ids = nullptr;  // [max_batch x kcap]
    int32_t kcap = 0;
  };
  struct Batch {
    Key key;
    int64_t nq = 0;
    int32_t kmax = 0;
    bool closed = false, done = false;
    int copying = 0;  // members still copying their queries in
    int members = 0;  // members that have not yet copied their rows out
    int status = 0;
    std::string err;
    Slab slab;
  };

  bool new_slab(Slab* s) {
    s->q = hooks_.alloc((size_t)max_batch_ * row_bytes_);
    if (!s->q) return false;
    if (!grow_slab(s, kInitialK)) {
      hooks_.release(s->q);
      s->q = nullptr;
      return false;
    }
    return true;
  }
  // only when a larger k arrives; the old contents are not needed
  bool grow_slab(Slab* s, int32_t k) {
    float* nd = (float*)hooks_.alloc((size_t)max_batch_ * k * sizeof(float));
    int64_t* ni =
        (int64_t*)hooks_.alloc((size_t)max_batch_ * k * sizeof(int64_t));
    if (!nd || !ni) {
      if (nd) hooks_.release(nd);
      if (ni) hooks_.release(ni);
      return false;
    }
    if (s->dist) hooks_.release(s->dist);
    if (s->ids) hooks_.release(s->ids);
    s->dist = nd;
    s->ids = ni;
    s->kcap = k;
    return true;
  }
  void drop_pool() {
    for (auto& s : pool_) {
      if (s.q) hooks_.release(s.q);
      if (s.dist) hooks_.release(s.dist);
      if (s.ids) hooks_.release(s.ids);
    }
    pool_.clear();
  }

  Hooks hooks_;
  std::mutex mu_;
  std::condition_variable cv_;
  bool enabled_ = false;
  bool flushing_ = false;
  int32_t max_batch_ = 0, max_wait_us_ = 0;
  size_t row_bytes_ = 0;
  int64_t inflight_ = 0;  // calls between joining a batch and leaving it
  std::deque<std::shared_ptr<Batch>> queue_;  // not yet flushing, oldest first
  std::vector<Slab> pool_;
  Stats stats_;
};

}  // namespace dgb
