// dg_shard.cpp — the sharded index (dg_sharded_*) and the stand-alone list
// merge (dg_merge_topk*) of include/dingo_gpu.h.  A dg_sharded is a set of
// ordinary dg_index shards plus the plumbing of one search: fan-out from
// persistent worker threads, gather into a slab on the merge device, and the
// rank-placement merge kernel (dgk::merge_lists).  Routing and the merge
// order live in dg_shard_core.h.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>

#include "dg_internal.h"
#include "dg_shard_core.h"

namespace {

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (dev >= 0 && dev != prev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// grow-only device buffer on the current device; the old block is freed
// after the stream that used it has drained
dg_status buf_reserve(dg_dbuf& b, size_t bytes, hipStream_t s) {
  if (bytes <= b.cap) {
    b.bytes = bytes;
    return DG_OK;
  }
  void* np = nullptr;
  if (hipMalloc(&np, bytes) != hipSuccess) {
    dg_set_error("hipMalloc(%zu) failed", bytes);
    return DG_ENOMEM;
  }
  if (b.p) {
    (void)hipStreamSynchronize(s);
    (void)hipFree(b.p);
  }
  b.p = np;
  b.cap = b.bytes = bytes;
  return DG_OK;
}

void buf_free(dg_dbuf& b) {
  if (b.p) (void)hipFree(b.p);
  b = {};
}

bool merge_args_ok(int32_t n_lists, int64_t nq, int32_t k_in, int32_t k_out,
                   int32_t metric) {
  if (n_lists < 1 || n_lists > 32 || k_in < 1 || k_in > 2048 || k_out < 1 ||
      k_out > 2048 || nq < 1 || metric < DG_METRIC_L2 ||
      metric > DG_METRIC_COSINE) {
    dg_set_error("bad merge args (need 1 <= n_lists <= 32, 1 <= k_in, k_out "
                 "<= 2048, nq >= 1, a float metric)");
    return false;
  }
  // one thread per input element, 256 per block, a 31-bit block count
  if (nq > ((int64_t)0x7fffffff * 256) / ((int64_t)n_lists * k_in)) {
    dg_set_error("merge of nq %lld x %d lists x %d exceeds one launch",
                 (long long)nq, n_lists, k_in);
    return false;
  }
  return true;
}

// One persistent thread per shard.  run() hands it one job and returns at
// once; wait() blocks until that job is done.
struct Worker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<void()> job;
  bool has_job = false, stop = false;

  void start() {
    th = std::thread([this] {
      std::unique_lock lk(mu);
      for (;;) {
        cv.wait(lk, [this] { return has_job || stop; });
        if (!has_job) return;  // stop, nothing pending
        std::function<void()> j = std::move(job);
        lk.unlock();
        j();
        lk.lock();
        has_job = false;
        cv.notify_all();
      }
    });
  }
  void run(std::function<void()> j) {
    std::lock_guard lk(mu);
    job = std::move(j);
    has_job = true;
    cv.notify_all();
  }
  void wait() {
    std::unique_lock lk(mu);
    cv.wait(lk, [this] { return !has_job; });
  }
  void join() {
    {
      std::lock_guard lk(mu);
      stop = true;
      cv.notify_all();
    }
    if (th.joinable()) th.join();
  }
};

// what one shard's job reports back (dg_last_error is per thread)
struct ShardResult {
  dg_status st = DG_OK;
  char msg[1024] = "";
};

}  // namespace

struct dg_sharded {
  dg_index_desc desc{};
  int32_t n = 0;
  std::vector<dg_index*> shards;
  std::vector<int> dev;        // device of shard i
  std::vector<int> leader;     // first shard on the same device
  std::vector<Worker*> workers;
  int merge_dev = 0;
  hipStream_t merge_stream = nullptr;
  hipEvent_t q_ready = nullptr;          // queries readable on merge device
  std::vector<hipEvent_t> q_copied;      // leader i: queries on its device
  std::vector<hipEvent_t> done;          // shard i: its slab slice written
  hipEvent_t ev_m0 = nullptr, ev_m1 = nullptr;  // around the merge kernel
  bool merge_timed = false;
  // merge device: gathered lists [S][nq][k] (dists, then ids) and the
  // staging of the host-pointer search
  dg_dbuf slab, h_in, h_dist, h_ids;
  // per shard off the merge device: its own result lists; per leader off the
  // merge device: the queries
  std::vector<dg_dbuf> loc_out, loc_q;
  std::shared_mutex rw;  // search shared; mutation, train exclusive
  std::mutex search_mu;  // slab, staging, workers and events are shared
};

namespace {

// runs fn(i) for every shard on the shard's worker, waits for all of them,
// and returns the first failure in shard order with its message
dg_status run_on_shards(dg_sharded* sh,
                        const std::function<dg_status(int32_t)>& fn,
                        const std::vector<char>* skip = nullptr) {
  std::vector<ShardResult> res(sh->n);
  for (int32_t i = 0; i < sh->n; i++) {
    if (skip && (*skip)[i]) continue;
    ShardResult* r = &res[i];
    sh->workers[i]->run([&fn, r, i] {
      r->st = fn(i);
      if (r->st != DG_OK) dg_last_error(r->msg, sizeof(r->msg));
    });
  }
  for (int32_t i = 0; i < sh->n; i++)
    if (!(skip && (*skip)[i])) sh->workers[i]->wait();
  for (int32_t i = 0; i < sh->n; i++)
    if (res[i].st != DG_OK) {
      dg_set_error("shard %d: %s", i, res[i].msg);
      return res[i].st;
    }
  return DG_OK;
}

bool is_trained(const dg_sharded* sh) {
  const dg_index* s0 = sh->shards[0];
  return s0->is_ready() &&
         (s0->desc.kind != DG_INDEX_IVF_PQ || s0->pq_trained);
}

// rows of one call, split by shard
struct Partition {
  std::vector<std::vector<int64_t>> ids;
  std::vector<std::vector<float>> x;
  std::vector<char> empty;
};

void partition_rows(const dg_sharded* sh, int64_t n, const int64_t* ids,
                    const float* x, Partition* p) {
  const int32_t d = sh->desc.d;
  p->ids.assign(sh->n, {});
  p->x.assign(sh->n, {});
  for (int64_t i = 0; i < n; i++) {
    const int32_t s = dg_shard_of(ids[i], sh->n);
    p->ids[s].push_back(ids[i]);
    if (x)
      p->x[s].insert(p->x[s].end(), x + (size_t)i * d,
                     x + (size_t)(i + 1) * d);
  }
  p->empty.assign(sh->n, 0);
  for (int32_t s = 0; s < sh->n; s++) p->empty[s] = p->ids[s].empty();
}

// negative ids and ids that occur twice in one call
dg_status check_batch_ids(int64_t n, const int64_t* ids) {
  std::unordered_map<int64_t, int32_t> batch;
  batch.reserve((size_t)n * 2);
  for (int64_t i = 0; i < n; i++) {
    if (ids[i] < 0) {
      dg_set_error("negative id %lld", (long long)ids[i]);
      return DG_EINVAL;
    }
    if (++batch[ids[i]] > 1) {
      dg_set_error("vector id duplicated in batch: %lld", (long long)ids[i]);
      return DG_EID_DUPLICATED;
    }
  }
  return DG_OK;
}

dg_status search_device_locked(dg_sharded* sh, int64_t nq, const float* d_x,
                               int32_t k, int32_t nprobe,
                               const dg_filter* filter, float* d_out_dist,
                               int64_t* d_out_ids) {
  const int32_t S = sh->n;
  const size_t list_elems = (size_t)nq * k;
  const size_t q_bytes = (size_t)nq * sh->desc.d * 4;
  DeviceGuard g(sh->merge_dev);
  dg_status st = buf_reserve(sh->slab, (size_t)S * list_elems * 12,
                             sh->merge_stream);
  if (st != DG_OK) return st;
  float* slab_d = (float*)sh->slab.p;
  int64_t* slab_i = (int64_t*)((char*)sh->slab.p + (size_t)S * list_elems * 4);
  // the queries are ready once the merge stream has reached this point
  DG_HIP_CHECK(hipEventRecord(sh->q_ready, sh->merge_stream));
  // one copy of the queries per distinct other device, on its leader's stream
  for (int32_t i = 0; i < S; i++) {
    if (sh->dev[i] == sh->merge_dev || sh->leader[i] != i) continue;
    DeviceGuard gi(sh->dev[i]);
    dg_index* ix = sh->shards[i];
    if ((st = buf_reserve(sh->loc_q[i], q_bytes, ix->stream)) != DG_OK)
      return st;
    DG_HIP_CHECK(hipStreamWaitEvent(ix->stream, sh->q_ready, 0));
    DG_HIP_CHECK(hipMemcpyPeerAsync(sh->loc_q[i].p, sh->dev[i], d_x,
                                    sh->merge_dev, q_bytes, ix->stream));
    DG_HIP_CHECK(hipEventRecord(sh->q_copied[i], ix->stream));
  }
  for (int32_t i = 0; i < S; i++) {
    if (sh->dev[i] == sh->merge_dev) continue;
    DeviceGuard gi(sh->dev[i]);
    if ((st = buf_reserve(sh->loc_out[i], list_elems * 12,
                          sh->shards[i]->stream)) != DG_OK)
      return st;
  }
  // fan out: dg_search_device may block the host on its non-fused paths, so
  // every shard's call is issued from the shard's own thread
  std::atomic<bool> failed{false};
  st = run_on_shards(sh, [&](int32_t i) -> dg_status {
    if (failed.load()) return DG_OK;  // nothing is started after a failure
    dg_index* ix = sh->shards[i];
    DeviceGuard gi(sh->dev[i]);
    const bool local = sh->dev[i] == sh->merge_dev;
    const float* q = local ? d_x : (const float*)sh->loc_q[sh->leader[i]].p;
    float* od = local ? slab_d + (size_t)i * list_elems
                      : (float*)sh->loc_out[i].p;
    int64_t* oi = local ? slab_i + (size_t)i * list_elems
                        : (int64_t*)((char*)sh->loc_out[i].p + list_elems * 4);
    dg_status s = DG_OK;
    hipError_t e = hipStreamWaitEvent(
        ix->stream, local ? sh->q_ready : sh->q_copied[sh->leader[i]], 0);
    if (e == hipSuccess) {
      s = dg_search_device(ix, nq, q, k, nprobe, filter, od, oi);
      if (s == DG_OK && !local) {
        e = hipMemcpyPeerAsync(slab_d + (size_t)i * list_elems, sh->merge_dev,
                               od, sh->dev[i], list_elems * 4, ix->stream);
        if (e == hipSuccess)
          e = hipMemcpyPeerAsync(slab_i + (size_t)i * list_elems,
                                 sh->merge_dev, oi, sh->dev[i],
                                 list_elems * 8, ix->stream);
      }
      if (s == DG_OK && e == hipSuccess)
        e = hipEventRecord(sh->done[i], ix->stream);
    }
    if (s == DG_OK && e != hipSuccess) {
      dg_set_error("HIP error %s in the fan-out: %s", hipGetErrorName(e),
                   hipGetErrorString(e));
      s = DG_EINTERNAL;
    }
    if (s != DG_OK) failed.store(true);
    return s;
  });
  if (st != DG_OK) {
    // no merge; drain what the other shards had enqueued, so that the next
    // search finds the slab and the local buffers idle
    for (int32_t i = 0; i < S; i++) {
      DeviceGuard gi(sh->dev[i]);
      (void)hipStreamSynchronize(sh->shards[i]->stream);
    }
    return st;
  }
  for (int32_t i = 0; i < S; i++)
    DG_HIP_CHECK(hipStreamWaitEvent(sh->merge_stream, sh->done[i], 0));
  DG_HIP_CHECK(hipEventRecord(sh->ev_m0, sh->merge_stream));
  dgk::merge_lists(sh->merge_stream, slab_d, slab_i, S, nq, k, k,
                   sh->desc.metric, d_out_dist, d_out_ids);
  DG_HIP_CHECK(hipGetLastError());
  DG_HIP_CHECK(hipEventRecord(sh->ev_m1, sh->merge_stream));
  sh->merge_timed = true;
  return DG_OK;
}

// argument rules shared by both search forms; *done = answered already
dg_status search_precheck(dg_sharded* sh, int64_t nq, const void* x,
                          int32_t k, const void* od, const void* oi,
                          bool* done) {
  *done = true;
  if (!sh || !x || !od || !oi || nq <= 0) {
    dg_set_error("bad search args");
    return DG_EINVAL;
  }
  if (k <= 0) return DG_OK;  // as dg_search: OK no-op
  if (k > 2048) {
    dg_set_error("k > 2048 not supported");
    return DG_ENOT_SUPPORT;
  }
  if (!merge_args_ok(sh->n, nq, k, k, sh->desc.metric)) return DG_EINVAL;
  *done = false;
  return DG_OK;
}

}  // namespace

// ---------------- stand-alone merge ----------------
extern "C" dg_status dg_merge_topk_device(int32_t n_lists, int64_t nq,
                                          int32_t k_in, int32_t k_out,
                                          int32_t metric,
                                          const float* d_dists,
                                          const int64_t* d_ids,
                                          float* d_out_dist,
                                          int64_t* d_out_ids, void* stream) {
  if (!d_dists || !d_ids || !d_out_dist || !d_out_ids) {
    dg_set_error("null arg");
    return DG_EINVAL;
  }
  if (!merge_args_ok(n_lists, nq, k_in, k_out, metric)) return DG_EINVAL;
  dgk::merge_lists((hipStream_t)stream, d_dists, d_ids, n_lists, nq, k_in,
                   k_out, metric, d_out_dist, d_out_ids);
  DG_HIP_CHECK(hipGetLastError());
  return DG_OK;
}

extern "C" dg_status dg_merge_topk(int32_t n_lists, int64_t nq, int32_t k_in,
                                   int32_t k_out, int32_t metric,
                                   const float* dists, const int64_t* ids,
                                   float* out_dist, int64_t* out_ids,
                                   int32_t device) {
  if (!dists || !ids || !out_dist || !out_ids) {
    dg_set_error("null arg");
    return DG_EINVAL;
  }
  if (!merge_args_ok(n_lists, nq, k_in, k_out, metric)) return DG_EINVAL;
  const int ndev = dg_device_count();
  if (ndev == 0) {
    dg_set_error("no HIP device (the GPU path has no CPU fallback)");
    return DG_ENOGPU;
  }
  if (device >= ndev) {
    dg_set_error("device %d out of range (%d visible)", device, ndev);
    return DG_EINVAL;
  }
  DeviceGuard g(device);
  const size_t n_in = (size_t)n_lists * nq * k_in, n_out = (size_t)nq * k_out;
  char* buf = nullptr;  // dists | out_dist | ids | out_ids, 8-byte aligned
  const size_t o_od = (n_in * 4 + 7) & ~(size_t)7;
  const size_t o_i = o_od + ((n_out * 4 + 7) & ~(size_t)7);
  const size_t o_oi = o_i + n_in * 8;
  if (hipMalloc((void**)&buf, o_oi + n_out * 8) != hipSuccess) {
    dg_set_error("hipMalloc(%zu) failed", o_oi + n_out * 8);
    return DG_ENOMEM;
  }
  hipError_t e = hipMemcpy(buf, dists, n_in * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(buf + o_i, ids, n_in * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    dgk::merge_lists(nullptr, (const float*)buf, (const int64_t*)(buf + o_i),
                     n_lists, nq, k_in, k_out, metric, (float*)(buf + o_od),
                     (int64_t*)(buf + o_oi));
    e = hipGetLastError();
  }
  // the blocking copies on the default stream wait for the kernel
  if (e == hipSuccess)
    e = hipMemcpy(out_dist, buf + o_od, n_out * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess)
    e = hipMemcpy(out_ids, buf + o_oi, n_out * 8, hipMemcpyDeviceToHost);
  (void)hipFree(buf);
  if (e != hipSuccess) {
    dg_set_error("HIP error %s in dg_merge_topk: %s", hipGetErrorName(e),
                 hipGetErrorString(e));
    return DG_EINTERNAL;
  }
  return DG_OK;
}

// ---------------- lifecycle ----------------
extern "C" void dg_sharded_destroy(dg_sharded* sh) {
  if (!sh) return;
  for (Worker* w : sh->workers) {
    w->join();
    delete w;
  }
  for (int32_t i = 0; i < (int32_t)sh->shards.size(); i++) {
    DeviceGuard g(sh->dev[i]);
    if (sh->shards[i]) (void)hipStreamSynchronize(sh->shards[i]->stream);
    if (i < (int32_t)sh->loc_out.size()) buf_free(sh->loc_out[i]);
    if (i < (int32_t)sh->loc_q.size()) buf_free(sh->loc_q[i]);
    if (i < (int32_t)sh->done.size() && sh->done[i])
      (void)hipEventDestroy(sh->done[i]);
    if (i < (int32_t)sh->q_copied.size() && sh->q_copied[i])
      (void)hipEventDestroy(sh->q_copied[i]);
  }
  {
    DeviceGuard g(sh->merge_dev);
    if (sh->merge_stream) (void)hipStreamSynchronize(sh->merge_stream);
    for (auto b : {&sh->slab, &sh->h_in, &sh->h_dist, &sh->h_ids})
      buf_free(*b);
    for (hipEvent_t e : {sh->q_ready, sh->ev_m0, sh->ev_m1})
      if (e) (void)hipEventDestroy(e);
    if (sh->merge_stream) (void)hipStreamDestroy(sh->merge_stream);
  }
  for (dg_index* ix : sh->shards) dg_index_destroy(ix);
  delete sh;
}

extern "C" dg_status dg_sharded_create(dg_sharded** out,
                                       const dg_index_desc* dp,
                                       int32_t n_shards,
                                       const int32_t* devices) {
  if (!out || !dp) {
    dg_set_error("null arg");
    return DG_EINVAL;
  }
  *out = nullptr;
  if (n_shards < 1 || n_shards > 32) {
    dg_set_error("n_shards %d out of range (need 1 <= n_shards <= 32)",
                 n_shards);
    return DG_EINVAL;
  }
  if (dg_kind_is_binary(dp->kind)) {
    dg_set_error("a sharded index holds float kinds only (kind %d)",
                 dp->kind);
    return DG_ENOT_SUPPORT;
  }
  if (dg_kind_is_hnsw(dp->kind)) {
    dg_set_error("a sharded index does not hold DG_INDEX_HNSW");
    return DG_ENOT_SUPPORT;
  }
  const int ndev = dg_device_count();
  if (ndev == 0) {
    dg_set_error("no HIP device (the GPU path has no CPU fallback)");
    return DG_ENOGPU;
  }
  for (int32_t i = 0; devices && i < n_shards; i++)
    if (devices[i] < 0 || devices[i] >= ndev) {
      dg_set_error("devices[%d] = %d out of range (%d visible)", i,
                   devices[i], ndev);
      return DG_EINVAL;
    }
  dg_sharded* sh = new dg_sharded();
  sh->n = n_shards;
  sh->desc = *dp;
  sh->dev.resize(n_shards);
  sh->leader.resize(n_shards);
  for (int32_t i = 0; i < n_shards; i++) {
    sh->dev[i] = devices ? devices[i] : 0;
    sh->leader[i] = i;
    for (int32_t j = 0; j < i; j++)
      if (sh->dev[j] == sh->dev[i]) {
        sh->leader[i] = j;
        break;
      }
  }
  sh->merge_dev = sh->dev[0];
  dg_index_desc sd = *dp;
  sd.reserve = dp->reserve > 0 ? (dp->reserve + n_shards - 1) / n_shards : 0;
  for (int32_t i = 0; i < n_shards; i++) {
    sd.device = sh->dev[i];
    dg_index* ix = nullptr;
    const dg_status st = dg_index_create(&ix, &sd);
    if (st != DG_OK) {  // the shard's own error text stands
      dg_sharded_destroy(sh);
      return st;
    }
    sh->shards.push_back(ix);
  }
  sh->done.assign(n_shards, nullptr);
  sh->q_copied.assign(n_shards, nullptr);
  sh->loc_out.resize(n_shards);
  sh->loc_q.resize(n_shards);
  bool ok = true;
  for (int32_t i = 0; i < n_shards && ok; i++) {
    DeviceGuard g(sh->dev[i]);
    ok = hipEventCreateWithFlags(&sh->done[i], hipEventDisableTiming) ==
             hipSuccess &&
         hipEventCreateWithFlags(&sh->q_copied[i], hipEventDisableTiming) ==
             hipSuccess;
  }
  if (ok) {
    DeviceGuard g(sh->merge_dev);
    ok = hipStreamCreate(&sh->merge_stream) == hipSuccess &&
         hipEventCreateWithFlags(&sh->q_ready, hipEventDisableTiming) ==
             hipSuccess &&
         hipEventCreate(&sh->ev_m0) == hipSuccess &&
         hipEventCreate(&sh->ev_m1) == hipSuccess;
  }
  if (!ok) {
    dg_set_error("stream/event init of the sharded index failed");
    dg_sharded_destroy(sh);
    return DG_EINTERNAL;
  }
  // the index's own description: defaults resolved as the shards did
  sh->desc.nlist = sh->shards[0]->desc.nlist;
  sh->desc.pq_m = sh->shards[0]->desc.pq_m;
  sh->desc.pq_nbits = sh->shards[0]->desc.pq_nbits;
  for (int32_t i = 0; i < n_shards; i++) {
    sh->workers.push_back(new Worker());
    sh->workers.back()->start();
  }
  *out = sh;
  return DG_OK;
}

extern "C" int32_t dg_sharded_n_shards(dg_sharded* sh) {
  return sh ? sh->n : 0;
}

extern "C" dg_index* dg_sharded_shard(dg_sharded* sh, int32_t i) {
  return sh && i >= 0 && i < sh->n ? sh->shards[i] : nullptr;
}

extern "C" dg_status dg_sharded_set_storage(dg_sharded* sh, int32_t storage) {
  if (!sh) return DG_EINVAL;
  std::unique_lock lk(sh->rw);
  // all or none: a shard that already holds rows would refuse
  for (dg_index* ix : sh->shards) {
    std::shared_lock sl(ix->rw);
    if (ix->ntotal != 0) {
      dg_set_error("dg_sharded_set_storage: the index already holds rows");
      return DG_EINVAL;
    }
  }
  for (dg_index* ix : sh->shards) {
    const dg_status st = dg_set_storage(ix, storage);
    if (st != DG_OK) return st;
  }
  return DG_OK;
}

extern "C" dg_status dg_sharded_set_sq_ranges(dg_sharded* sh,
                                              const float* vmin,
                                              const float* vdiff) {
  if (!sh) return DG_EINVAL;
  std::unique_lock lk(sh->rw);
  for (dg_index* ix : sh->shards) {
    const dg_status st = dg_set_sq_ranges(ix, vmin, vdiff);
    if (st != DG_OK) return st;
  }
  return DG_OK;
}

extern "C" dg_status dg_sharded_get_sq_ranges(dg_sharded* sh, float* vmin,
                                              float* vdiff) {
  if (!sh) return DG_EINVAL;
  std::shared_lock lk(sh->rw);
  return dg_get_sq_ranges(sh->shards[0], vmin, vdiff);
}

// ---------------- train / structure ----------------
static dg_status replicate_from_shard0(dg_sharded* sh) {
  dg_index* s0 = sh->shards[0];
  const int32_t nlist = s0->desc.nlist, d = sh->desc.d;
  std::vector<float> cents((size_t)nlist * d);
  dg_status st = dg_get_centroids(s0, cents.data());
  if (st != DG_OK) return st;
  std::vector<float> cb;
  const bool pq = s0->desc.kind == DG_INDEX_IVF_PQ;
  if (pq) {
    cb.resize((size_t)dg_pq_ksub(s0->desc) * d);  // m * ksub * (d / m)
    if ((st = dg_get_codebooks(s0, cb.data())) != DG_OK) return st;
  }
  // SQ8: shard 0's ranges go to every shard bit for bit, like the centroids
  const bool sq8 = dg_get_storage(s0) == DG_STORAGE_SQ8;
  std::vector<float> rng;
  if (sq8) {
    rng.resize((size_t)2 * d);
    if ((st = dg_get_sq_ranges(s0, rng.data(), rng.data() + d)) != DG_OK)
      return st;
  }
  for (int32_t i = 1; i < sh->n; i++) {
    if ((st = dg_set_centroids(sh->shards[i], nlist, cents.data())) != DG_OK)
      return st;
    if (pq && (st = dg_set_codebooks(sh->shards[i], s0->desc.pq_m,
                                     s0->desc.pq_nbits, cb.data())) != DG_OK)
      return st;
    if (sq8 && (st = dg_set_sq_ranges(sh->shards[i], rng.data(),
                                      rng.data() + d)) != DG_OK)
      return st;
  }
  sh->desc.nlist = nlist;
  return DG_OK;
}

extern "C" dg_status dg_sharded_train(dg_sharded* sh, int64_t n,
                                      const float* x) {
  if (!sh) return DG_EINVAL;
  std::unique_lock lk(sh->rw);
  if (sh->desc.kind != DG_INDEX_FLAT && is_trained(sh)) return DG_OK;
  dg_status st = dg_train(sh->shards[0], n, x);
  if (st != DG_OK || sh->desc.kind == DG_INDEX_FLAT) return st;
  return replicate_from_shard0(sh);
}

extern "C" dg_status dg_sharded_set_centroids(dg_sharded* sh, int32_t nlist,
                                              const float* centroids) {
  if (!sh) return DG_EINVAL;
  std::unique_lock lk(sh->rw);
  for (dg_index* ix : sh->shards) {
    const dg_status st = dg_set_centroids(ix, nlist, centroids);
    if (st != DG_OK) return st;
  }
  sh->desc.nlist = nlist;
  return DG_OK;
}

extern "C" dg_status dg_sharded_get_centroids(dg_sharded* sh, float* out) {
  if (!sh) return DG_EINVAL;
  std::shared_lock lk(sh->rw);
  return dg_get_centroids(sh->shards[0], out);
}

extern "C" dg_status dg_sharded_set_codebooks(dg_sharded* sh, int32_t m,
                                              int32_t nbits,
                                              const float* codebooks) {
  if (!sh) return DG_EINVAL;
  std::unique_lock lk(sh->rw);
  for (dg_index* ix : sh->shards) {
    const dg_status st = dg_set_codebooks(ix, m, nbits, codebooks);
    if (st != DG_OK) return st;
  }
  return DG_OK;
}

extern "C" dg_status dg_sharded_get_codebooks(dg_sharded* sh, float* out) {
  if (!sh) return DG_EINVAL;
  std::shared_lock lk(sh->rw);
  return dg_get_codebooks(sh->shards[0], out);
}

// ---------------- mutation ----------------
static dg_status add_or_upsert(dg_sharded* sh, int64_t n, const int64_t* ids,
                               const float* x, bool upsert) {
  if (!sh || !ids || !x || n <= 0) {
    dg_set_error("bad add args");
    return DG_EINVAL;
  }
  std::unique_lock lk(sh->rw);
  if (!is_trained(sh)) {
    dg_set_error("IVF index not trained (EVECTOR_NOT_TRAIN)");
    return DG_ENOT_TRAINED;
  }
  dg_status st = check_batch_ids(n, ids);
  if (st != DG_OK) return st;
  if (!upsert)
    for (int64_t i = 0; i < n; i++)
      if (dg_contains_id(sh->shards[dg_shard_of(ids[i], sh->n)], ids[i])) {
        dg_set_error("vector id duplicated: %lld (EVECTOR_ID_DUPLICATED)",
                     (long long)ids[i]);
        return DG_EID_DUPLICATED;
      }
  Partition p;
  partition_rows(sh, n, ids, x, &p);
  return run_on_shards(
      sh,
      [&](int32_t i) {
        const int64_t ni = (int64_t)p.ids[i].size();
        return upsert ? dg_upsert(sh->shards[i], ni, p.ids[i].data(),
                                  p.x[i].data())
                      : dg_add(sh->shards[i], ni, p.ids[i].data(),
                               p.x[i].data());
      },
      &p.empty);
}

extern "C" dg_status dg_sharded_add(dg_sharded* sh, int64_t n,
                                    const int64_t* ids, const float* x) {
  return add_or_upsert(sh, n, ids, x, false);
}

extern "C" dg_status dg_sharded_upsert(dg_sharded* sh, int64_t n,
                                       const int64_t* ids, const float* x) {
  return add_or_upsert(sh, n, ids, x, true);
}

extern "C" dg_status dg_sharded_remove(dg_sharded* sh, int64_t n,
                                       const int64_t* ids) {
  if (!sh || !ids || n <= 0) return DG_EINVAL;
  std::unique_lock lk(sh->rw);
  // all must exist on their shards, else nothing is removed anywhere
  for (int64_t i = 0; i < n; i++)
    if (ids[i] < 0 ||
        !dg_contains_id(sh->shards[dg_shard_of(ids[i], sh->n)], ids[i])) {
      dg_set_error("remove not found vector id %lld (EVECTOR_INVALID)",
                   (long long)ids[i]);
      return DG_ENOT_FOUND;
    }
  Partition p;
  partition_rows(sh, n, ids, nullptr, &p);
  return run_on_shards(
      sh,
      [&](int32_t i) {
        return dg_remove(sh->shards[i], (int64_t)p.ids[i].size(),
                         p.ids[i].data());
      },
      &p.empty);
}

// ---------------- search ----------------
extern "C" dg_status dg_sharded_search_device(dg_sharded* sh, int64_t nq,
                                              const float* d_x, int32_t k,
                                              int32_t nprobe,
                                              const dg_filter* filter,
                                              float* d_out_dist,
                                              int64_t* d_out_ids) {
  bool answered;
  const dg_status st =
      search_precheck(sh, nq, d_x, k, d_out_dist, d_out_ids, &answered);
  if (answered) return st;
  std::shared_lock lk(sh->rw);
  std::lock_guard sg(sh->search_mu);
  return search_device_locked(sh, nq, d_x, k, nprobe, filter, d_out_dist,
                              d_out_ids);
}

extern "C" dg_status dg_sharded_search(dg_sharded* sh, int64_t nq,
                                       const float* x, int32_t k,
                                       int32_t nprobe, const dg_filter* filter,
                                       float* out_dist, int64_t* out_ids) {
  bool answered;
  dg_status st = search_precheck(sh, nq, x, k, out_dist, out_ids, &answered);
  if (answered) return st;
  std::shared_lock lk(sh->rw);
  std::lock_guard sg(sh->search_mu);
  DeviceGuard g(sh->merge_dev);
  const size_t q_bytes = (size_t)nq * sh->desc.d * 4;
  const size_t n_out = (size_t)nq * k;
  if ((st = buf_reserve(sh->h_in, q_bytes, sh->merge_stream)) != DG_OK ||
      (st = buf_reserve(sh->h_dist, n_out * 4, sh->merge_stream)) != DG_OK ||
      (st = buf_reserve(sh->h_ids, n_out * 8, sh->merge_stream)) != DG_OK)
    return st;
  DG_HIP_CHECK(hipMemcpyAsync(sh->h_in.p, x, q_bytes, hipMemcpyHostToDevice,
                              sh->merge_stream));
  st = search_device_locked(sh, nq, (const float*)sh->h_in.p, k, nprobe,
                            filter, (float*)sh->h_dist.p,
                            (int64_t*)sh->h_ids.p);
  if (st != DG_OK) return st;
  DG_HIP_CHECK(hipMemcpyAsync(out_dist, sh->h_dist.p, n_out * 4,
                              hipMemcpyDeviceToHost, sh->merge_stream));
  DG_HIP_CHECK(hipMemcpyAsync(out_ids, sh->h_ids.p, n_out * 8,
                              hipMemcpyDeviceToHost, sh->merge_stream));
  DG_HIP_CHECK(hipStreamSynchronize(sh->merge_stream));
  return DG_OK;
}

extern "C" dg_status dg_sharded_sync(dg_sharded* sh) {
  if (!sh) return DG_EINVAL;
  DeviceGuard g(sh->merge_dev);
  DG_HIP_CHECK(hipStreamSynchronize(sh->merge_stream));
  return DG_OK;
}

// ---------------- range search ----------------
extern "C" dg_status dg_sharded_range_search(dg_sharded* sh, int64_t nq,
                                             const float* x, float radius,
                                             const dg_filter* filter,
                                             int64_t* lims, int64_t** out_ids,
                                             float** out_dists) {
  if (out_ids) *out_ids = nullptr;  // always safe to hand to dg_free
  if (out_dists) *out_dists = nullptr;
  if (!sh || !x || !lims || !out_ids || !out_dists || nq <= 0) {
    dg_set_error("bad range search args");
    return DG_EINVAL;
  }
  std::shared_lock lk(sh->rw);
  std::lock_guard sg(sh->search_mu);
  const int32_t S = sh->n;
  std::vector<std::vector<int64_t>> s_lims(S,
                                           std::vector<int64_t>(nq + 1, 0));
  std::vector<int64_t*> s_ids(S, nullptr);
  std::vector<float*> s_dists(S, nullptr);
  dg_status st = run_on_shards(sh, [&](int32_t i) {
    return dg_range_search(sh->shards[i], nq, x, radius, filter,
                           s_lims[i].data(), &s_ids[i], &s_dists[i]);
  });
  if (st == DG_OK) {
    int64_t total = 0;
    for (int32_t i = 0; i < S; i++) total += s_lims[i][nq];
    *out_ids = (int64_t*)malloc((size_t)std::max<int64_t>(total, 1) * 8);
    *out_dists = (float*)malloc((size_t)std::max<int64_t>(total, 1) * 4);
    if (!*out_ids || !*out_dists) {
      free(*out_ids);
      free(*out_dists);
      *out_ids = nullptr;
      *out_dists = nullptr;
      dg_set_error("out of host memory for %lld range results",
                   (long long)total);
      st = DG_ENOMEM;
    }
  }
  if (st == DG_OK) {
    const bool l2 = sh->desc.metric == DG_METRIC_L2;
    std::vector<std::pair<float, int64_t>> rows;
    int64_t w = 0;
    lims[0] = 0;
    for (int64_t q = 0; q < nq; q++) {
      rows.clear();
      for (int32_t i = 0; i < S; i++)
        for (int64_t j = s_lims[i][q]; j < s_lims[i][q + 1]; j++)
          rows.emplace_back(s_dists[i][j], s_ids[i][j]);
      // best first (L2 ascending, IP / COSINE descending), ties toward the
      // smaller id: the order of dg_range_search
      std::sort(rows.begin(), rows.end(),
                [l2](const std::pair<float, int64_t>& a,
                     const std::pair<float, int64_t>& b) {
                  if (a.first != b.first)
                    return l2 ? a.first < b.first : a.first > b.first;
                  return a.second < b.second;
                });
      for (const auto& r : rows) {
        (*out_dists)[w] = r.first;
        (*out_ids)[w++] = r.second;
      }
      lims[q + 1] = w;
    }
  }
  for (int32_t i = 0; i < S; i++) {
    free(s_ids[i]);
    free(s_dists[i]);
  }
  return st;
}

// ---------------- stats ----------------
extern "C" dg_status dg_sharded_stats(dg_sharded* sh, dg_stats_out* out) {
  if (!sh || !out) return DG_EINVAL;
  std::shared_lock lk(sh->rw);
  std::lock_guard sg(sh->search_mu);
  memset(out, 0, sizeof(*out));
  for (int32_t i = 0; i < sh->n; i++) {
    dg_stats_out s;
    const dg_status st = dg_stats(sh->shards[i], &s);
    if (st != DG_OK) return st;
    if (i == 0) {
      out->d = s.d;
      out->metric = s.metric;
      out->kind = s.kind;
      out->nlist = s.nlist;
      out->is_trained = s.is_trained;
    }
    out->ntotal += s.ntotal;
    out->device_bytes += s.device_bytes;
    out->deleted_count += s.deleted_count;
    out->last_scan_bytes_algorithmic += s.last_scan_bytes_algorithmic;
    out->last_coarse_ms = std::max(out->last_coarse_ms, s.last_coarse_ms);
    out->last_scan_ms = std::max(out->last_scan_ms, s.last_scan_ms);
    out->last_select_ms = std::max(out->last_select_ms, s.last_select_ms);
    out->last_total_ms = std::max(out->last_total_ms, s.last_total_ms);
    out->last_nq = std::max(out->last_nq, s.last_nq);
  }
  if (sh->merge_timed) {
    DeviceGuard g(sh->merge_dev);
    float ms = 0;
    if (hipEventSynchronize(sh->ev_m1) == hipSuccess &&
        hipEventElapsedTime(&ms, sh->ev_m0, sh->ev_m1) == hipSuccess) {
      out->last_select_ms += ms;
      out->last_total_ms += ms;
    }
  }
  if (out->last_scan_ms > 0)
    out->last_scan_gbps_algorithmic =
        (double)out->last_scan_bytes_algorithmic / (out->last_scan_ms * 1e6);
  return DG_OK;
}
