// dg_hnsw.cpp — DG_INDEX_HNSW: the host graph (dg_hnsw_core.h), its device
// mirror and the entry points around k_hnsw_search (hnsw.hip.cpp).
//
// The graph and the rows live on the host (the sequential build reads them)
// and are mirrored on the device before the first search after a mutation:
// rows are appended (only the new ones travel), the graph arrays are uploaded
// whole.  The generic entry points of dg_abi.cpp dispatch here by kind.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "dg_internal.h"
#include "dg_hnsw_core.h"

namespace {

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

// the visited bitmaps of one launch stay below this many bytes; a batch is
// split into as many launches as that takes
constexpr size_t kVisitedBytesMax = (size_t)256 << 20;
// DG_HNSW_VISITED_BYTES lowers the bound (tests: a batch of a few dozen
// queries then takes several launches); read per call, like DG_SCAN_FUSED
size_t visited_bytes_max() {
  const char* e = getenv("DG_HNSW_VISITED_BYTES");
  if (!e || !*e) return kVisitedBytesMax;
  const long long v = atoll(e);
  return v > 0 && (size_t)v < kVisitedBytesMax ? (size_t)v : kVisitedBytesMax;
}

}  // namespace

struct dg_hnsw_state {
  dg_hnsw::Graph g;
  dg_hnsw::Visited vis;
  std::unordered_map<int64_t, uint32_t> live;  // id -> node
  int32_t ef_search = 10;
  // device mirror
  bool dirty = true;       // the graph arrays differ from the host's
  int64_t dev_rows = 0;    // rows already on the device
  dg_dbuf d_rows, d_cnt0, d_links0, d_levels, d_up_off, d_up_cnt, d_up_links,
      d_ids, d_pass_ids, d_deleted, d_pass, d_vis, d_ctr, d_fids;
  // counters of the last search (expansions, dist_evals, flag), copied here
  // behind its kernels
  int64_t* h_ctr = nullptr;  // pinned, 3 entries
  bool searched = false;

  std::vector<dg_dbuf*> mirror() {
    return {&d_rows, &d_cnt0, &d_links0, &d_levels, &d_up_off, &d_up_cnt,
            &d_up_links, &d_ids, &d_pass_ids, &d_deleted};
  }
};

namespace {

dg_status reserve(dg_index* ix, dg_dbuf& b, size_t bytes, bool keep) {
  if (bytes <= b.cap) {
    b.bytes = bytes;
    return DG_OK;
  }
  const size_t newcap = std::max(bytes, b.cap + b.cap / 2);
  void* np = nullptr;
  if (hipMalloc(&np, newcap) != hipSuccess) {
    dg_set_error("hipMalloc(%zu) failed", newcap);
    return DG_ENOMEM;
  }
  if (keep && b.p && b.bytes &&
      hipMemcpyAsync(np, b.p, b.bytes, hipMemcpyDeviceToDevice,
                     ix->stream) != hipSuccess) {
    (void)hipFree(np);
    dg_set_error("grow copy failed");
    return DG_EINTERNAL;
  }
  if (b.p) {
    (void)hipStreamSynchronize(ix->stream);
    (void)hipFree(b.p);
  }
  b.p = np;
  b.cap = newcap;
  b.bytes = bytes;
  return DG_OK;
}

template <class T>
dg_status upload(dg_index* ix, dg_dbuf& b, const std::vector<T>& v) {
  const size_t bytes = v.size() * sizeof(T);
  dg_status st = reserve(ix, b, std::max<size_t>(bytes, 16), false);
  if (st != DG_OK) return st;
  if (bytes)
    DG_HIP_CHECK(hipMemcpyAsync(b.p, v.data(), bytes, hipMemcpyHostToDevice,
                                ix->stream));
  return DG_OK;
}

// caller holds the write lock
dg_status upload_mirror(dg_index* ix) {
  dg_hnsw_state* h = ix->hnsw;
  const dg_hnsw::Graph& g = h->g;
  const int32_t du = ix->d_user, dp = ix->desc.d;
  dg_status st = reserve(ix, h->d_rows,
                         std::max<size_t>((size_t)g.n * dp * 4, 16), true);
  if (st != DG_OK) return st;
  if (g.n > h->dev_rows) {
    float* dst = (float*)h->d_rows.p + (size_t)h->dev_rows * dp;
    const float* src = g.row(h->dev_rows);
    const size_t rows = (size_t)(g.n - h->dev_rows);
    if (du == dp) {
      DG_HIP_CHECK(hipMemcpyAsync(dst, src, rows * dp * 4,
                                  hipMemcpyHostToDevice, ix->stream));
    } else {
      DG_HIP_CHECK(hipMemsetAsync(dst, 0, rows * dp * 4, ix->stream));
      DG_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dp * 4, src, (size_t)du * 4,
                                    (size_t)du * 4, rows,
                                    hipMemcpyHostToDevice, ix->stream));
    }
  }
  // the bitmap kernel's convention: a negative id is a tombstone
  std::vector<int64_t> pass_ids(g.ids);
  for (int64_t i = 0; i < g.n; i++)
    if (g.deleted[i]) pass_ids[i] = -2;
  if ((st = upload(ix, h->d_cnt0, g.cnt0)) != DG_OK ||
      (st = upload(ix, h->d_links0, g.links0)) != DG_OK ||
      (st = upload(ix, h->d_levels, g.levels)) != DG_OK ||
      (st = upload(ix, h->d_up_off, g.up_off)) != DG_OK ||
      (st = upload(ix, h->d_up_cnt, g.up_cnt)) != DG_OK ||
      (st = upload(ix, h->d_up_links, g.up_links)) != DG_OK ||
      (st = upload(ix, h->d_ids, g.ids)) != DG_OK ||
      (st = upload(ix, h->d_deleted, g.deleted)) != DG_OK ||
      (st = upload(ix, h->d_pass_ids, pass_ids)) != DG_OK)
    return st;
  // the sources are pageable host vectors: wait before they can change
  DG_HIP_CHECK(hipStreamSynchronize(ix->stream));
  h->dev_rows = g.n;
  h->dirty = false;
  return DG_OK;
}

// Takes lk (shared) with the device mirror equal to the host graph.  The
// test of `dirty` and the use of the mirror fall under ONE acquisition: a
// mutation that slips in while the lock is dropped for the upload sets
// `dirty` again and the loop uploads again.  On failure lk is not held.
dg_status lock_clean(dg_index* ix, std::shared_lock<std::shared_mutex>& lk) {
  for (;;) {
    lk.lock();
    if (!ix->hnsw->dirty) return DG_OK;
    lk.unlock();
    std::unique_lock wl(ix->rw);
    if (ix->hnsw->dirty) {
      const dg_status st = upload_mirror(ix);
      if (st != DG_OK) return st;
    }
  }
}

// the bounds of a search, checked before anything is staged or launched
dg_status check_search_args(int32_t k, int32_t ef_search) {
  if (ef_search < 0 || ef_search > dg_hnsw::kMaxEfSearch) {
    dg_set_error("ef_search %d outside 0..1024", ef_search);
    return DG_EINVAL;
  }
  if (k > dg_hnsw::kMaxEfSearch) {
    dg_set_error("HNSW search: k > 1024 not supported");
    return DG_ENOT_SUPPORT;
  }
  return DG_OK;
}

bool is_hnsw(dg_index* ix, const char* fn) {
  if (ix && ix->hnsw) return true;
  dg_set_error("%s: not a DG_INDEX_HNSW index", fn);
  return false;
}

dg_status report_flag(dg_index* ix) {
  if (ix->hnsw->searched && ix->hnsw->h_ctr[2] != 0) {
    dg_set_error("k_hnsw_search met a link out of range or its iteration "
                 "cap: the graph on the device is corrupt");
    return DG_EINTERNAL;
  }
  return DG_OK;
}

}  // namespace

dg_status dg_hnsw_create_state(dg_index* ix) {
  dg_hnsw_state* h = new dg_hnsw_state();
  h->g.configure(ix->d_user, ix->desc.metric, 32, 200, 100);
  if (hipHostMalloc((void**)&h->h_ctr, 3 * sizeof(int64_t)) != hipSuccess) {
    delete h;
    dg_set_error("hipHostMalloc failed");
    return DG_ENOMEM;
  }
  h->h_ctr[0] = h->h_ctr[1] = h->h_ctr[2] = 0;
  ix->hnsw = h;
  return DG_OK;
}

void dg_hnsw_destroy_state(dg_index* ix) {
  dg_hnsw_state* h = ix->hnsw;
  if (!h) return;
  for (dg_dbuf* b : h->mirror())
    if (b->p) (void)hipFree(b->p);
  for (dg_dbuf* b : {&h->d_pass, &h->d_vis, &h->d_ctr, &h->d_fids})
    if (b->p) (void)hipFree(b->p);
  if (h->h_ctr) (void)hipHostFree(h->h_ctr);
  delete h;
  ix->hnsw = nullptr;
}

extern "C" dg_status dg_hnsw_configure(dg_index* ix, int32_t nlinks,
                                       int32_t ef_construction,
                                       uint64_t seed) {
  if (!is_hnsw(ix, "dg_hnsw_configure")) return DG_EINVAL;
  std::unique_lock lk(ix->rw);
  if (ix->hnsw->g.n != 0) {
    dg_set_error("dg_hnsw_configure: the index already holds nodes");
    return DG_EINVAL;
  }
  if (nlinks < dg_hnsw::kMinLinks || nlinks > dg_hnsw::kMaxLinks ||
      ef_construction < 1 || ef_construction > dg_hnsw::kMaxEfConstruction) {
    dg_set_error("dg_hnsw_configure: nlinks %d (2..128) or ef_construction "
                 "%d (1..4096) unsupported", nlinks, ef_construction);
    return DG_ENOT_SUPPORT;
  }
  const int64_t max_elements = ix->hnsw->g.max_elements;
  ix->hnsw->g = dg_hnsw::Graph();
  ix->hnsw->g.configure(ix->d_user, ix->desc.metric, nlinks, ef_construction,
                        seed);
  ix->hnsw->g.max_elements = max_elements;
  ix->hnsw->dirty = true;
  return DG_OK;
}

extern "C" dg_status dg_hnsw_set_ef(dg_index* ix, int32_t ef_search) {
  if (!is_hnsw(ix, "dg_hnsw_set_ef")) return DG_EINVAL;
  if (ef_search < 1 || ef_search > dg_hnsw::kMaxEfSearch) {
    dg_set_error("dg_hnsw_set_ef: ef_search %d outside 1..1024", ef_search);
    return DG_EINVAL;
  }
  std::unique_lock lk(ix->rw);
  ix->hnsw->ef_search = ef_search;
  return DG_OK;
}

extern "C" dg_status dg_hnsw_get_info(dg_index* ix, dg_hnsw_info* out) {
  if (!is_hnsw(ix, "dg_hnsw_get_info") || !out) return DG_EINVAL;
  std::shared_lock lk(ix->rw);
  const dg_hnsw::Graph& g = ix->hnsw->g;
  memset(out, 0, sizeof(*out));
  out->nlinks = g.M;
  out->max_m0 = g.maxM0;
  out->ef_construction = g.ef_construction;
  out->ef_search = ix->hnsw->ef_search;
  out->max_level = g.max_level;
  out->entry_point = g.entry;
  out->n_nodes = g.n;
  out->n_deleted = g.n_deleted;
  out->seed = g.seed;
  return DG_OK;
}

dg_status dg_hnsw_add(dg_index* ix, int64_t n, const int64_t* ids,
                      const float* x, bool x_on_device, bool upsert) {
  dg_hnsw_state* h = ix->hnsw;
  const int32_t d = ix->d_user;
  DevGuard dg(ix->device);
  std::vector<float> host;
  if (x_on_device) {  // the build runs on the host
    host.resize((size_t)n * d);
    DG_HIP_CHECK(hipMemcpy(host.data(), x, host.size() * 4,
                           hipMemcpyDeviceToHost));
    x = host.data();
  }
  std::unique_lock lk(ix->rw);
  dg_hnsw::Graph& g = h->g;
  for (int64_t i = 0; i < n; i++) {
    if (ids[i] < 0) {
      dg_set_error("negative id %lld", (long long)ids[i]);
      return DG_EINVAL;
    }
    if (!upsert && h->live.count(ids[i])) {
      dg_set_error("vector id duplicated: %lld (EVECTOR_ID_DUPLICATED)",
                   (long long)ids[i]);
      return DG_EID_DUPLICATED;
    }
  }
  {
    std::unordered_map<int64_t, int32_t> batch;
    for (int64_t i = 0; i < n; i++)
      if (++batch[ids[i]] > 1) {
        dg_set_error("vector id duplicated in batch: %lld",
                     (long long)ids[i]);
        return DG_EID_DUPLICATED;
      }
  }
  for (size_t i = 0; i < (size_t)n * d; i++)
    if (!std::isfinite(x[i])) {
      dg_set_error("row %lld has a NaN or infinite component",
                   (long long)(i / d));
      return DG_EINVAL;
    }
  if ((uint64_t)(g.n + n) > 0xfffffff0ull) {
    dg_set_error("an HNSW index holds at most 2^32 - 16 nodes");
    return DG_ENOT_SUPPORT;
  }
  std::vector<float> row(d);
  for (int64_t i = 0; i < n; i++) {
    auto it = h->live.find(ids[i]);
    if (it != h->live.end()) {  // upsert: tombstone the old node
      g.deleted[it->second] = 1;
      g.n_deleted++;
      h->live.erase(it);
    }
    const float* src = x + (size_t)i * d;
    if (g.metric == dg_hnsw::kMetricCosine) {
      dg_hnsw::normalize(src, d, row.data());
      src = row.data();
    }
    h->live[ids[i]] = (uint32_t)dg_hnsw::insert(g, ids[i], src, h->vis);
  }
  h->dirty = true;
  ix->ntotal = g.n;
  ix->n_deleted = g.n_deleted;
  return DG_OK;
}

dg_status dg_hnsw_remove(dg_index* ix, int64_t n, const int64_t* ids) {
  dg_hnsw_state* h = ix->hnsw;
  std::unique_lock lk(ix->rw);
  std::unordered_map<int64_t, int32_t> batch;
  for (int64_t i = 0; i < n; i++)
    if (!h->live.count(ids[i]) || ++batch[ids[i]] > 1) {
      dg_set_error("remove not found vector id %lld (EVECTOR_INVALID)",
                   (long long)ids[i]);
      return DG_ENOT_FOUND;
    }
  for (int64_t i = 0; i < n; i++) {
    auto it = h->live.find(ids[i]);
    h->g.deleted[it->second] = 1;  // hnswlib markDelete
    h->g.n_deleted++;
    h->live.erase(it);
  }
  h->dirty = true;
  ix->n_deleted = h->g.n_deleted;
  return DG_OK;
}

dg_status dg_hnsw_reconstruct(dg_index* ix, int64_t n, const int64_t* ids,
                              float* out) {
  dg_hnsw_state* h = ix->hnsw;
  std::shared_lock lk(ix->rw);
  for (int64_t i = 0; i < n; i++)
    if (!h->live.count(ids[i])) {
      dg_set_error("reconstruct not found vector id %lld",
                   (long long)ids[i]);
      return DG_ENOT_FOUND;
    }
  const int32_t d = ix->d_user;
  for (int64_t i = 0; i < n; i++)
    memcpy(out + (size_t)i * d, h->g.row(h->live[ids[i]]), (size_t)d * 4);
  return DG_OK;
}

bool dg_hnsw_contains_id(dg_index* ix, int64_t id) {
  std::shared_lock lk(ix->rw);
  return ix->hnsw->live.count(id) != 0;
}

extern "C" dg_status dg_search_hnsw_device(dg_index* ix, int64_t nq,
                                           const float* d_x, int32_t k,
                                           int32_t ef_search,
                                           const dg_filter* filter,
                                           float* d_out_dist,
                                           int64_t* d_out_ids) {
  if (!ix || !d_x || !d_out_dist || !d_out_ids || nq <= 0) {
    dg_set_error("bad search args");
    return DG_EINVAL;
  }
  if (!is_hnsw(ix, "dg_search_hnsw_device")) return DG_EINVAL;
  if (k <= 0) return DG_OK;
  dg_status st = check_search_args(k, ef_search);
  if (st != DG_OK) return st;
  if (nq > 0x7fffffff) {
    dg_set_error("nq %lld per call unsupported", (long long)nq);
    return DG_EINVAL;
  }
  dg_hnsw_state* h = ix->hnsw;
  DevGuard dg(ix->device);
  std::shared_lock lk(ix->rw, std::defer_lock);
  if ((st = lock_clean(ix, lk)) != DG_OK) return st;
  std::lock_guard sg(ix->search_mu);
  const dg_hnsw::Graph& g = h->g;
  if (g.n == 0) {
    (void)hipMemsetAsync(d_out_dist, 0, (size_t)nq * k * 4, ix->stream);
    (void)hipMemsetAsync(d_out_ids, 0xff, (size_t)nq * k * 8, ix->stream);
    h->searched = false;
    ix->times.last_nq = 0;
    return DG_OK;
  }
  const int32_t efp = std::max(ef_search > 0 ? ef_search : h->ef_search, k);
  (void)hipEventRecord(ix->ev[0], ix->stream);

  // filter -> device form -> pass bitmap over the nodes (tombstones are
  // negative ids in d_pass_ids)
  dg_dev_filter df{};
  df.kind = DG_FILTER_NONE;
  if (filter && filter->kind != DG_FILTER_NONE) {
    df.kind = filter->kind;
    df.negate = filter->negate;
    df.min_id = filter->min_id;
    df.max_id = filter->max_id;
    if (filter->kind == DG_FILTER_SORTED_IDS) {
      if ((st = reserve(ix, h->d_fids,
                        std::max<size_t>((size_t)filter->n_ids * 8, 16),
                        false)) != DG_OK)
        return st;
      if (filter->n_ids > 0)
        DG_HIP_CHECK(hipMemcpyAsync(h->d_fids.p, filter->ids,
                                    (size_t)filter->n_ids * 8,
                                    hipMemcpyHostToDevice, ix->stream));
      df.ids = (const int64_t*)h->d_fids.p;
      df.n_ids = filter->n_ids;
    } else if (filter->kind == DG_FILTER_BITMAP) {
      const size_t words = (size_t)((filter->bitmap_nbits + 63) / 64);
      if ((st = reserve(ix, h->d_fids, std::max<size_t>(words * 8, 16),
                        false)) != DG_OK)
        return st;
      if (words)
        DG_HIP_CHECK(hipMemcpyAsync(h->d_fids.p, filter->bitmap, words * 8,
                                    hipMemcpyHostToDevice, ix->stream));
      df.bitmap = (const uint64_t*)h->d_fids.p;
      df.bitmap_base = filter->bitmap_base;
      df.bitmap_nbits = filter->bitmap_nbits;
    }
  }
  const int64_t vwords = (g.n + 31) / 32;
  if ((st = reserve(ix, h->d_pass, (size_t)vwords * 4, false)) != DG_OK ||
      (st = reserve(ix, h->d_ctr, 32, false)) != DG_OK)
    return st;
  dgk::build_pass_bitmap(ix->stream, (const int64_t*)h->d_pass_ids.p, g.n,
                         &df, (uint32_t*)h->d_pass.p);
  const int64_t per_launch = std::max<int64_t>(
      1, std::min<int64_t>(nq, (int64_t)(visited_bytes_max() /
                                         ((size_t)vwords * 4))));
  if ((st = reserve(ix, h->d_vis, (size_t)per_launch * vwords * 4, false)) !=
      DG_OK)
    return st;
  DG_HIP_CHECK(hipMemsetAsync(h->d_ctr.p, 0, 32, ix->stream));

  dgk::hnsw_graph dev{};
  dev.rows = (const float*)h->d_rows.p;
  dev.cnt0 = (const int32_t*)h->d_cnt0.p;
  dev.links0 = (const uint32_t*)h->d_links0.p;
  dev.levels = (const int32_t*)h->d_levels.p;
  dev.up_off = (const int64_t*)h->d_up_off.p;
  dev.up_cnt = (const int32_t*)h->d_up_cnt.p;
  dev.up_links = (const uint32_t*)h->d_up_links.p;
  dev.pass = (const uint32_t*)h->d_pass.p;
  dev.ids = (const int64_t*)h->d_ids.p;
  dev.n = g.n;
  dev.entry = g.entry;
  dev.d = ix->desc.d;
  dev.maxM = g.maxM;
  dev.maxM0 = g.maxM0;
  dev.max_level = g.max_level;
  dev.metric = g.metric;
  // ev[2]..ev[3] is last_scan_ms: the kernel alone when the batch takes one
  // launch (the rule); a batch split over several launches also counts the
  // clears of the visited workspace between them
  for (int64_t q0 = 0; q0 < nq; q0 += per_launch) {
    const int64_t qn = std::min(per_launch, nq - q0);
    DG_HIP_CHECK(hipMemsetAsync(h->d_vis.p, 0, (size_t)qn * vwords * 4,
                                ix->stream));
    if (q0 == 0) {
      (void)hipEventRecord(ix->ev[1], ix->stream);
      (void)hipEventRecord(ix->ev[2], ix->stream);
    }
    dgk::hnsw_search(ix->stream, dev, d_x + q0 * ix->d_user, qn, ix->d_user,
                     k, efp, (uint32_t*)h->d_vis.p, vwords,
                     d_out_dist + q0 * k, d_out_ids + q0 * k,
                     (unsigned long long*)h->d_ctr.p,
                     (int32_t*)((char*)h->d_ctr.p + 16));
  }
  DG_HIP_CHECK(hipGetLastError());
  (void)hipEventRecord(ix->ev[3], ix->stream);
  // counters and the flag follow the kernels into pinned memory
  DG_HIP_CHECK(hipMemcpyAsync(h->h_ctr, h->d_ctr.p, 24,
                              hipMemcpyDeviceToHost, ix->stream));
  (void)hipEventRecord(ix->ev[4], ix->stream);
  h->searched = true;
  ix->times.last_nq = nq;
  ix->times.scan_split = false;
  return DG_OK;
}

extern "C" dg_status dg_search_hnsw(dg_index* ix, int64_t nq, const float* x,
                                    int32_t k, int32_t ef_search,
                                    const dg_filter* filter, float* out_dist,
                                    int64_t* out_ids) {
  if (!ix || !x || !out_dist || !out_ids || nq <= 0) {
    dg_set_error("bad search args");
    return DG_EINVAL;
  }
  if (!is_hnsw(ix, "dg_search_hnsw")) return DG_EINVAL;
  return dg_hnsw_search_host(ix, nq, x, k, ef_search, filter, out_dist,
                             out_ids);
}

// after the host form's synchronise
dg_status dg_hnsw_after_sync(dg_index* ix) { return report_flag(ix); }

dg_status dg_hnsw_check_search_args(int32_t k, int32_t ef_search) {
  return check_search_args(k, ef_search);
}

extern "C" dg_status dg_hnsw_last_counters(dg_index* ix, int64_t* expansions,
                                           int64_t* dist_evals) {
  if (!is_hnsw(ix, "dg_hnsw_last_counters")) return DG_EINVAL;
  DevGuard dg(ix->device);
  std::lock_guard sg(ix->search_mu);
  DG_HIP_CHECK(hipStreamSynchronize(ix->stream));
  const bool have = ix->hnsw->searched;
  if (expansions) *expansions = have ? ix->hnsw->h_ctr[0] : 0;
  if (dist_evals) *dist_evals = have ? ix->hnsw->h_ctr[1] : 0;
  return report_flag(ix);
}

dg_status dg_hnsw_stats(dg_index* ix, dg_stats_out* out) {
  dg_hnsw_state* h = ix->hnsw;
  std::shared_lock lk(ix->rw);
  DevGuard dg(ix->device);
  memset(out, 0, sizeof(*out));
  out->ntotal = h->g.n - h->g.n_deleted;
  out->d = ix->d_user;
  out->metric = ix->desc.metric;
  out->kind = ix->desc.kind;
  out->nlist = 0;
  out->is_trained = 1;
  size_t db = 0;
  for (dg_dbuf* b : h->mirror()) db += b->cap;
  out->device_bytes = (int64_t)db;
  out->deleted_count = h->g.n_deleted;
  if (ix->times.last_nq > 0) {
    std::lock_guard sg(ix->search_mu);
    (void)hipEventSynchronize(ix->ev[4]);
    float ms01 = 0, ms23 = 0, ms04 = 0;
    (void)hipEventElapsedTime(&ms01, ix->ev[0], ix->ev[1]);
    (void)hipEventElapsedTime(&ms23, ix->ev[2], ix->ev[3]);
    (void)hipEventElapsedTime(&ms04, ix->ev[0], ix->ev[4]);
    out->last_coarse_ms = ms01;
    out->last_scan_ms = ms23;
    out->last_total_ms = ms04;
    out->last_select_ms = std::max(0.0f, ms04 - ms23 - ms01);
    out->last_nq = ix->times.last_nq;
    out->last_scan_bytes_algorithmic = h->h_ctr[1] * 4 * (int64_t)ix->d_user;
    if (ms23 > 0)
      out->last_scan_gbps_algorithmic =
          (double)out->last_scan_bytes_algorithmic / (ms23 * 1e6);
    return report_flag(ix);
  }
  return DG_OK;
}

// ---- export: the DEVICE copy, so an upload bug shows as one ----
extern "C" dg_status dg_hnsw_export_nodes(dg_index* ix, int64_t* ids,
                                          uint8_t* deleted, int32_t* levels) {
  if (!is_hnsw(ix, "dg_hnsw_export_nodes")) return DG_EINVAL;
  DevGuard dg(ix->device);
  std::shared_lock lk(ix->rw, std::defer_lock);
  dg_status st = lock_clean(ix, lk);
  if (st != DG_OK) return st;
  dg_hnsw_state* h = ix->hnsw;
  const size_t n = (size_t)h->g.n;
  if (n == 0) return DG_OK;
  if (ids)
    DG_HIP_CHECK(hipMemcpy(ids, h->d_ids.p, n * 8, hipMemcpyDeviceToHost));
  if (deleted)
    DG_HIP_CHECK(hipMemcpy(deleted, h->d_deleted.p, n,
                           hipMemcpyDeviceToHost));
  if (levels)
    DG_HIP_CHECK(hipMemcpy(levels, h->d_levels.p, n * 4,
                           hipMemcpyDeviceToHost));
  return DG_OK;
}

extern "C" dg_status dg_hnsw_export_level(dg_index* ix, int32_t level,
                                          int32_t* counts, uint32_t* links) {
  if (!is_hnsw(ix, "dg_hnsw_export_level") || !counts || !links)
    return DG_EINVAL;
  DevGuard dg(ix->device);
  std::shared_lock lk(ix->rw, std::defer_lock);
  dg_status st = lock_clean(ix, lk);
  if (st != DG_OK) return st;
  dg_hnsw_state* h = ix->hnsw;
  const dg_hnsw::Graph& g = h->g;
  if (level < 0 || level > std::max(g.max_level, 0)) {
    dg_set_error("dg_hnsw_export_level: level %d outside 0..%d", level,
                 std::max(g.max_level, 0));
    return DG_EINVAL;
  }
  const size_t n = (size_t)g.n;
  if (n == 0) return DG_OK;
  if (level == 0) {
    DG_HIP_CHECK(hipMemcpy(counts, h->d_cnt0.p, n * 4,
                           hipMemcpyDeviceToHost));
    DG_HIP_CHECK(hipMemcpy(links, h->d_links0.p, n * g.maxM0 * 4,
                           hipMemcpyDeviceToHost));
    return DG_OK;
  }
  std::vector<int32_t> lv(n), uc(g.up_cnt.size());
  std::vector<int64_t> off(n + 1);
  std::vector<uint32_t> ul(g.up_links.size());
  DG_HIP_CHECK(hipMemcpy(lv.data(), h->d_levels.p, n * 4,
                         hipMemcpyDeviceToHost));
  DG_HIP_CHECK(hipMemcpy(off.data(), h->d_up_off.p, (n + 1) * 8,
                         hipMemcpyDeviceToHost));
  if (!uc.empty()) {
    DG_HIP_CHECK(hipMemcpy(uc.data(), h->d_up_cnt.p, uc.size() * 4,
                           hipMemcpyDeviceToHost));
    DG_HIP_CHECK(hipMemcpy(ul.data(), h->d_up_links.p, ul.size() * 4,
                           hipMemcpyDeviceToHost));
  }
  memset(links, 0, n * g.maxM * 4);
  for (size_t i = 0; i < n; i++) {
    counts[i] = -1;
    if (lv[i] < level) continue;
    const int64_t at = off[i] + level - 1;
    if (at < 0 || at >= (int64_t)uc.size()) {
      dg_set_error("dg_hnsw_export_level: offsets on the device are corrupt");
      return DG_EINTERNAL;
    }
    counts[i] = uc[at];
    memcpy(links + i * g.maxM, &ul[(size_t)at * g.maxM], (size_t)g.maxM * 4);
  }
  return DG_OK;
}

// ---- hnswlib container ----
extern "C" dg_status dg_save_hnswlib(dg_index* ix, const char* path) {
  if (!is_hnsw(ix, "dg_save_hnswlib") || !path) return DG_EINVAL;
  std::vector<uint8_t> bytes;
  {
    std::shared_lock lk(ix->rw);
    dg_hnsw::save(ix->hnsw->g, bytes);
  }
  FILE* f = fopen(path, "wb");
  if (!f) {
    dg_set_error("cannot open %s for writing", path);
    return DG_EIO;
  }
  const bool ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  if (fclose(f) != 0 || !ok) {
    dg_set_error("short write to %s", path);
    return DG_EIO;
  }
  return DG_OK;
}

extern "C" dg_status dg_load_hnswlib(dg_index** out, const char* path,
                                     int32_t metric, int32_t d,
                                     int32_t device) {
  if (!out || !path) {
    dg_set_error("null arg");
    return DG_EINVAL;
  }
  if (metric < DG_METRIC_L2 || metric > DG_METRIC_COSINE || d <= 0 ||
      d > 8192) {
    dg_set_error("dg_load_hnswlib: bad metric %d or d %d", metric, d);
    return DG_EINVAL;
  }
  FILE* f = fopen(path, "rb");
  if (!f) {
    dg_set_error("cannot open %s", path);
    return DG_EIO;
  }
  std::vector<uint8_t> bytes;
  uint8_t buf[1 << 16];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, f)) > 0)
    bytes.insert(bytes.end(), buf, buf + got);
  fclose(f);
  // everything is checked before the first device call
  dg_hnsw::Graph g;
  std::string err;
  const int rc = dg_hnsw::load(bytes.data(), bytes.size(), metric, d, g, err);
  if (rc != dg_hnsw::kOk) {
    dg_set_error("%s", err.c_str());
    return (dg_status)rc;
  }
  dg_index_desc desc{};
  desc.kind = DG_INDEX_HNSW;
  desc.metric = metric;
  desc.d = d;
  desc.device = device;
  dg_index* ix = nullptr;
  dg_status st = dg_index_create(&ix, &desc);
  if (st != DG_OK) return st;
  dg_hnsw_state* h = ix->hnsw;
  h->g = std::move(g);
  for (int64_t i = 0; i < h->g.n; i++)
    if (!h->g.deleted[i]) h->live[h->g.ids[i]] = (uint32_t)i;
  h->dirty = true;
  ix->ntotal = h->g.n;
  ix->n_deleted = h->g.n_deleted;
  *out = ix;
  return DG_OK;
}

// the container's max_elements field (include/dingo_gpu.h)
extern "C" int64_t dg_hnsw_max_elements(dg_index* ix, int64_t set) {
  if (!ix || !ix->hnsw) return -1;
  std::unique_lock lk(ix->rw);
  if (set >= 0) ix->hnsw->g.max_elements = set;
  return ix->hnsw->g.max_elements;
}
