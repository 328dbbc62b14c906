// batch_core_test.cpp — drives dg_batch_core.h (the queue logic of
// dg_search_batched) on the CPU with a fake device.  Stand-alone: build with
// a C++17 compiler and -pthread, optionally with -fsanitize=thread or
// -fsanitize=address,undefined; exit status 0 means every check held.
//
// The fake flush answers row r of a batch with f(query row, column) and
// sleeps a little, so batches form while it "runs".  A query row carries a
// token that is unique to its call and row, plus the key and k of its call,
// which lets the flush itself check that a batch is homogeneous.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <set>
#include <thread>
#include <vector>

#include "../../dingo-store_amd/csrc/dg_batch_core.h"

namespace {

constexpr int kThreads = 32;
constexpr int kCallsPerThread = 150;
constexpr int32_t kMaxBatch = 8;
constexpr int kInjectedStatus = 77;
constexpr int64_t kFailFlush = 40;  // the flush that fails (counted from 1)

struct Row {  // one query row, row_bytes = sizeof(Row)
  int64_t token;
  int32_t nprobe, filter_kind, k, pad;
};

std::atomic<int> g_fail{0};
#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, \
              #c);                                                   \
      g_fail++;                                                      \
    }                                                                \
  } while (0)

float f_dist(int64_t token, int j) { return (float)(token % 100003) + 0.5f * j; }
int64_t f_id(int64_t token, int j) { return token * 4096 + j; }

std::atomic<int> g_in_flush{0};
std::atomic<int64_t> g_flushes{0}, g_flush_rows{0}, g_max_rows{0};
std::atomic<int64_t> g_allocs{0}, g_frees{0};
std::mutex g_failed_mu;
std::set<int64_t> g_failed_tokens;  // rows of the failed flush

int fake_flush(const dgb::Flush& f, std::string* err) {
  CHECK(g_in_flush.fetch_add(1) == 0);  // flushes never overlap
  const int64_t n = g_flushes.fetch_add(1) + 1;
  g_flush_rows += f.nq;
  int64_t m = g_max_rows.load();
  while (f.nq > m && !g_max_rows.compare_exchange_weak(m, f.nq)) {
  }
  CHECK(f.nq >= 1 && f.nq <= kMaxBatch);
  const Row* rows = (const Row*)f.q;
  int32_t kmax = 0;
  for (int64_t r = 0; r < f.nq; r++) {
    CHECK(rows[r].nprobe == f.key.nprobe);
    CHECK(rows[r].filter_kind == f.key.filter_kind);
    kmax = std::max(kmax, rows[r].k);
  }
  CHECK(kmax == f.k);  // the batch runs at the largest k of its members
  std::this_thread::sleep_for(std::chrono::microseconds(60));
  int st = 0;
  if (n == kFailFlush) {
    std::lock_guard<std::mutex> lk(g_failed_mu);
    for (int64_t r = 0; r < f.nq; r++) g_failed_tokens.insert(rows[r].token);
    *err = "injected failure of flush " + std::to_string(n);
    st = kInjectedStatus;
  } else {
    for (int64_t r = 0; r < f.nq; r++)
      for (int j = 0; j < f.k; j++) {
        f.dist[r * f.k + j] = f_dist(rows[r].token, j);
        f.ids[r * f.k + j] = f_id(rows[r].token, j);
      }
  }
  g_in_flush--;
  return st;
}

struct Tally {
  std::atomic<int64_t> ok{0}, failed{0}, bypassed{0}, passthrough{0},
      ok_rows{0}, bypass_rows{0}, failed_rows{0};
};
std::mutex g_seen_mu;
std::set<int64_t> g_seen_failed_tokens;  // rows of calls that got the error

void worker(dgb::Batcher* b, int tid, int ncalls, std::atomic<int64_t>* done,
            Tally* t) {
  std::mt19937 rng(1000 + tid);
  const int32_t ks[] = {1, 5, 10, 16, 200};  // 200 > kInitialK: slabs grow
  std::vector<Row> q;
  std::vector<float> dist;
  std::vector<int64_t> ids;
  for (int c = 0; c < ncalls; c++) {
    int64_t nq = 1 + rng() % 3;
    const uint32_t dice = rng() % 40;
    if (dice == 0) nq = kMaxBatch;      // at max_batch: bypass
    if (dice == 1) nq = kMaxBatch + 3;  // above it: bypass
    const int32_t k = ks[rng() % (rng() % 8 ? 4 : 5)];
    dgb::Key key;
    key.nprobe = (rng() % 2) ? 4 : 8;
    if (rng() % 3 == 0) {
      key.filter_kind = 1;
      key.min_id = 0;
      key.max_id = 100;
    }
    q.resize(nq);
    for (int64_t r = 0; r < nq; r++) {
      q[r].token = ((int64_t)tid * 100000 + c) * 16 + r + 1;
      q[r].nprobe = key.nprobe;
      q[r].filter_kind = key.filter_kind;
      q[r].k = k;
      q[r].pad = 0;
    }
    dist.assign((size_t)nq * k, -1.f);
    ids.assign((size_t)nq * k, -7);
    std::string err;
    const int st =
        b->submit(q.data(), nq, k, key, dist.data(), ids.data(), &err);
    if (st == 0) {
      t->ok++;
      t->ok_rows += nq;
      bool good = true;  // exactly the caller's own rows
      for (int64_t r = 0; r < nq; r++)
        for (int j = 0; j < k; j++)
          good = good && dist[r * k + j] == f_dist(q[r].token, j) &&
                 ids[r * k + j] == f_id(q[r].token, j);
      CHECK(good);
    } else if (st == kInjectedStatus) {
      t->failed++;
      t->failed_rows += nq;
      CHECK(err == "injected failure of flush " + std::to_string(kFailFlush));
      CHECK(ids[0] == -7);  // nothing was written
      std::lock_guard<std::mutex> lk(g_seen_mu);
      for (int64_t r = 0; r < nq; r++) g_seen_failed_tokens.insert(q[r].token);
    } else if (st == dgb::kBypassed) {
      t->bypassed++;
      t->bypass_rows += nq;
      CHECK(nq >= kMaxBatch);
    } else if (st == dgb::kNotEnabled) {
      t->passthrough++;
    } else {
      CHECK(!"unexpected status");
    }
    (*done)++;
  }
}

}  // namespace

int main() {
  dgb::Hooks hooks;
  hooks.alloc = [](size_t n) {
    g_allocs++;
    return malloc(n);
  };
  hooks.release = [](void* p) {
    g_frees++;
    free(p);
  };
  hooks.flush = fake_flush;
  {
    dgb::Batcher b(hooks);

    // not enabled: nothing is queued or counted
    {
      Row r{1, 4, 0, 1, 0};
      float d;
      int64_t i;
      std::string err;
      CHECK(b.submit(&r, 1, 1, dgb::Key(), &d, &i, &err) == dgb::kNotEnabled);
      CHECK(!b.note_bypass(1));
      CHECK(b.stats().calls == 0);
    }

    // ---- phase A: zero wait, 32 threads, disable under traffic ----
    CHECK(b.enable(kMaxBatch, 0, sizeof(Row)));
    Tally ta;
    std::atomic<int64_t> done{0};
    std::vector<std::thread> th;
    for (int i = 0; i < kThreads; i++)
      th.emplace_back(worker, &b, i, kCallsPerThread, &done, &ta);
    const int64_t total = (int64_t)kThreads * kCallsPerThread;
    while (done.load() < total * 2 / 3) std::this_thread::yield();
    b.disable();  // returns once every batched call has left
    const dgb::Stats sa = b.stats();
    const int64_t flushes_at_disable = g_flushes.load();
    CHECK(g_in_flush.load() == 0);
    for (auto& t : th) t.join();
    // after disable nothing was batched any more
    CHECK(g_flushes.load() == flushes_at_disable);
    const dgb::Stats sb = b.stats();
    CHECK(sb.calls == sa.calls && sb.flushes == sa.flushes);
    CHECK(ta.passthrough.load() > 0);
    CHECK(ta.ok + ta.failed + ta.bypassed + ta.passthrough == total);
    CHECK(sa.calls == ta.ok + ta.failed + ta.bypassed);
    CHECK(sa.queries == ta.ok_rows + ta.failed_rows + ta.bypass_rows);
    CHECK(sa.bypassed == ta.bypassed && ta.bypassed.load() > 0);
    CHECK(sa.flushes == g_flushes.load());
    CHECK(g_flush_rows.load() == ta.ok_rows + ta.failed_rows);
    CHECK(sa.max_flush_queries == g_max_rows.load());
    CHECK(sa.max_flush_queries >= 2 && sa.max_flush_queries <= kMaxBatch);
    CHECK(sa.flushes < ta.ok + ta.failed);  // batches did form
    // the injected failure reached its members, all of them, and nobody else
    CHECK(g_flushes.load() >= kFailFlush);
    CHECK(ta.failed.load() >= 1);
    CHECK(!g_failed_tokens.empty());
    CHECK(g_failed_tokens == g_seen_failed_tokens);
    printf("phase A: %lld calls, %lld ok, %lld failed, %lld bypassed, %lld "
           "after disable; %lld flushes, largest %lld rows\n",
           (long long)total, (long long)ta.ok, (long long)ta.failed,
           (long long)ta.bypassed, (long long)ta.passthrough,
           (long long)sa.flushes, (long long)sa.max_flush_queries);

    // ---- phase B: enabled again, with a wait for company ----
    CHECK(b.enable(kMaxBatch, 200, sizeof(Row)));
    CHECK(b.stats().calls == 0);  // statistics start over
    Tally tb;
    std::atomic<int64_t> done_b{0};
    th.clear();
    for (int i = 0; i < 8; i++)
      th.emplace_back(worker, &b, 100 + i, 100, &done_b, &tb);
    for (auto& t : th) t.join();
    const dgb::Stats sc = b.stats();
    CHECK(tb.failed == 0 && tb.passthrough == 0);
    CHECK(tb.ok + tb.bypassed == 800);
    CHECK(sc.calls == 800 && sc.bypassed == tb.bypassed);
    CHECK(sc.flushes < tb.ok);
    printf("phase B: 800 calls, %lld flushes, largest %lld rows\n",
           (long long)sc.flushes, (long long)sc.max_flush_queries);

    // a lone caller is not held up: no company, no wait beyond max_wait_us
    Row r{5, 4, 0, 3, 0};
    float d[3];
    int64_t i3[3];
    std::string err;
    CHECK(b.submit(&r, 1, 3, dgb::Key{4, 0, 0, 0, 0}, d, i3, &err) == 0);
    CHECK(i3[2] == f_id(5, 2) && d[1] == f_dist(5, 1));
  }
  CHECK(g_allocs.load() == g_frees.load());  // the destructor frees the slabs
  if (g_fail.load()) {
    fprintf(stderr, "FAILED: %d checks\n", g_fail.load());
    return 1;
  }
  printf("OK\n");
  return 0;
}
