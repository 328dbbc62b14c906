// dg_hnsw_core.h — the host side of the HNSW index (DG_INDEX_HNSW): the
// graph, hnswlib's sequential insertion, the reference search that
// k_hnsw_search restates, and the hnswlib saveIndex container.  Host-only, no
// HIP include: tests/host/hnsw_core_test.cpp compiles it stand-alone.
// DESIGN.md §HNSW has the definitions and the arguments.
//
// Order: everything is compared as the pair (key, internal node), ascending,
// packed into one u64 (order-preserving image of the f32 key << 32 | node).
// key = sum (q - x)^2 for L2 and 0 - sum q * x for IP / cosine (0 - s, not -s:
// a zero dot gives +0.0, so the bit image orders exactly like the float).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace dg_hnsw {

// the dg_status values the container reader answers with
enum { kOk = 0, kNotSupport = 3, kEio = 6 };
enum { kMetricL2 = 0, kMetricIp = 1, kMetricCosine = 2 };
constexpr int32_t kMinLinks = 2, kMaxLinks = 128;
constexpr int32_t kMaxEfConstruction = 4096, kMaxEfSearch = 1024;

static inline uint32_t enc_f32(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return (int32_t)u < 0 ? ~u : (u | 0x80000000u);
}
static inline float dec_f32(uint32_t e) {
  uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e;
  float x;
  memcpy(&x, &u, 4);
  return x;
}
static inline uint64_t pack(float key, uint32_t node) {
  return ((uint64_t)enc_f32(key) << 32) | node;
}
static inline uint32_t node_of(uint64_t p) { return (uint32_t)p; }
static inline float key_of(uint64_t p) { return dec_f32((uint32_t)(p >> 32)); }

static inline uint64_t splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// x / (sqrtf(sum x^2) + 1e-30f): the reference's NormalizeVectorForHnsw
static inline void normalize(const float* x, int32_t d, float* out) {
  float s = 0.0f;
  for (int32_t j = 0; j < d; j++) s += x[j] * x[j];
  const float inv = 1.0f / (sqrtf(s) + 1e-30f);
  for (int32_t j = 0; j < d; j++) out[j] = x[j] * inv;
}

struct Graph {
  int32_t d = 0, metric = kMetricL2;
  int32_t M = 32, maxM = 32, maxM0 = 64, ef_construction = 200;
  uint64_t seed = 100;
  double mult = 1.0 / std::log(32.0);
  int64_t max_elements = 0;  // the container's field; 0 = n at save
  int64_t n = 0, n_deleted = 0;
  int32_t max_level = -1;
  int64_t entry = -1;
  std::vector<float> rows;       // [n][d], arrival order (a second copy of
                                 // the device rows: the build reads them)
  std::vector<int64_t> ids;      // external id
  std::vector<uint8_t> deleted;  // hnswlib's markDelete
  std::vector<int32_t> levels;
  std::vector<int32_t> cnt0;     // level 0: count[n], links[n][maxM0]
  std::vector<uint32_t> links0;
  // levels >= 1: node i owns the lists up_off[i] .. up_off[i + 1), one per
  // level 1 .. levels[i], each a count and maxM link slots
  std::vector<int64_t> up_off;   // [n + 1]
  std::vector<int32_t> up_cnt;
  std::vector<uint32_t> up_links;

  void configure(int32_t d_, int32_t metric_, int32_t nlinks, int32_t efc,
                 uint64_t seed_) {
    d = d_;
    metric = metric_;
    M = maxM = nlinks;
    maxM0 = 2 * nlinks;
    ef_construction = efc;
    seed = seed_;
    mult = 1.0 / std::log((double)nlinks);
    up_off.assign(1, 0);
  }
  const float* row(int64_t i) const { return rows.data() + i * d; }
  int32_t cap(int32_t level) const { return level == 0 ? maxM0 : maxM; }
  int32_t* cnt(int64_t i, int32_t level) {
    return level == 0 ? &cnt0[i] : &up_cnt[up_off[i] + level - 1];
  }
  uint32_t* links(int64_t i, int32_t level) {
    return level == 0 ? &links0[i * maxM0]
                      : &up_links[(up_off[i] + level - 1) * maxM];
  }
  int32_t cnt(int64_t i, int32_t level) const {
    return const_cast<Graph*>(this)->cnt(i, level)[0];
  }
  const uint32_t* links(int64_t i, int32_t level) const {
    return const_cast<Graph*>(this)->links(i, level);
  }
  size_t graph_bytes() const {
    return ids.size() * 8 + deleted.size() + levels.size() * 4 +
           cnt0.size() * 4 + links0.size() * 4 + up_off.size() * 8 +
           up_cnt.size() * 4 + up_links.size() * 4;
  }
};

// 16 independent partial sums (so the host build vectorises), added in a
// fixed order: the same inputs give the same float on every host
static inline float key_rows(int32_t metric, const float* q, const float* x,
                             int32_t d) {
  float acc[16] = {0};
  int32_t j = 0;
  if (metric == kMetricL2) {
    for (; j + 16 <= d; j += 16)
      for (int t = 0; t < 16; t++) {
        const float df = q[j + t] - x[j + t];
        acc[t] += df * df;
      }
    for (int t = 0; j < d; j++, t++) {
      const float df = q[j] - x[j];
      acc[t] += df * df;
    }
  } else {
    for (; j + 16 <= d; j += 16)
      for (int t = 0; t < 16; t++) acc[t] += q[j + t] * x[j + t];
    for (int t = 0; j < d; j++, t++) acc[t] += q[j] * x[j];
  }
  float s = 0.0f;
  for (int t = 0; t < 16; t++) s += acc[t];
  return metric == kMetricL2 ? s : 0.0f - s;
}

struct Counters {
  int64_t expansions = 0, dist_evals = 0;
};

// visited set with an epoch stamp per node (no clearing between searches)
struct Visited {
  std::vector<uint32_t> stamp;
  uint32_t epoch = 0;
  void begin(int64_t n) {
    if ((int64_t)stamp.size() < n) stamp.resize(n, 0);
    if (++epoch == 0) {
      std::fill(stamp.begin(), stamp.end(), 0);
      epoch = 1;
    }
  }
  bool test_set(uint32_t i) {
    if (stamp[i] == epoch) return true;
    stamp[i] = epoch;
    return false;
  }
};

static inline void sorted_insert(std::vector<uint64_t>& a, uint64_t x) {
  a.insert(std::lower_bound(a.begin(), a.end(), x), x);
}

// greedy step loop of the upper levels: move to the smallest of cur and its
// neighbours at `level` until cur is that smallest
static inline uint64_t greedy(const Graph& g, const float* q, uint64_t cur,
                              int32_t level, Counters* ctr) {
  for (;;) {
    uint64_t best = cur;
    const uint32_t c = node_of(cur);
    const int32_t m = g.cnt(c, level);
    const uint32_t* l = g.links(c, level);
    for (int32_t t = 0; t < m; t++) {
      const uint64_t p = pack(key_rows(g.metric, q, g.row(l[t]), g.d), l[t]);
      if (ctr) ctr->dist_evals++;
      best = std::min(best, p);
    }
    if (best == cur) return cur;
    cur = best;
  }
}

// The beam of one level ("level 0"): W receives the ef
// smallest admissible nodes found, ascending.  pass = null admits every node
// that is not deleted.
static inline void beam(const Graph& g, const float* q, uint64_t ep,
                        int32_t level, int32_t ef, const uint8_t* pass,
                        Visited& vis, std::vector<uint64_t>& W,
                        Counters* ctr) {
  auto admissible = [&](uint32_t e) {
    return !g.deleted[e] && (!pass || pass[e]);
  };
  std::vector<uint64_t> C;
  W.clear();
  vis.begin(g.n);
  vis.test_set(node_of(ep));
  C.push_back(ep);
  if (admissible(node_of(ep))) W.push_back(ep);
  std::vector<uint64_t> fresh;
  while (!C.empty()) {
    if ((int32_t)W.size() == ef && C.front() > W.back()) break;
    const uint32_t c = node_of(C.front());
    C.erase(C.begin());
    if (ctr) ctr->expansions++;
    const int32_t m = g.cnt(c, level);
    const uint32_t* l = g.links(c, level);
    fresh.clear();
    for (int32_t t = 0; t < m; t++) {
      if (vis.test_set(l[t])) continue;
      fresh.push_back(pack(key_rows(g.metric, q, g.row(l[t]), g.d), l[t]));
      if (ctr) ctr->dist_evals++;
    }
    for (uint64_t e : fresh) {
      if ((int32_t)W.size() < ef || e < W.back()) {
        if ((int32_t)C.size() < ef) {
          sorted_insert(C, e);
        } else if (e < C.back()) {
          C.pop_back();
          sorted_insert(C, e);
        }
        if (admissible(node_of(e))) {
          sorted_insert(W, e);
          if ((int32_t)W.size() > ef) W.pop_back();
        }
      }
    }
  }
}

// The reference search of one query.  out_ids receive INTERNAL nodes (-1
// padding), out_keys the keys (0.0f padding).
static inline void search(const Graph& g, const float* q, int32_t k,
                          int32_t ef, const uint8_t* pass, Visited& vis,
                          int64_t* out_nodes, float* out_keys,
                          Counters* ctr) {
  for (int32_t i = 0; i < k; i++) {
    out_nodes[i] = -1;
    out_keys[i] = 0.0f;
  }
  if (g.n == 0 || g.entry < 0) return;
  const int32_t efp = std::max(ef, k);
  uint64_t cur = pack(key_rows(g.metric, q, g.row(g.entry), g.d),
                      (uint32_t)g.entry);
  if (ctr) ctr->dist_evals++;
  for (int32_t l = g.max_level; l >= 1; l--) cur = greedy(g, q, cur, l, ctr);
  std::vector<uint64_t> W;
  beam(g, q, cur, 0, efp, pass, vis, W, ctr);
  for (int32_t i = 0; i < k && i < (int32_t)W.size(); i++) {
    out_nodes[i] = node_of(W[i]);
    out_keys[i] = key_of(W[i]);
  }
}

// ---- insertion (hnswlib addPoint) ----

static inline int32_t draw_level(const Graph& g, int64_t node) {
  const uint64_t r = splitmix64(g.seed + (uint64_t)node);
  const double u = (double)((r >> 11) + 1) * (1.0 / 9007199254740992.0);
  return (int32_t)std::floor(-std::log(u) * g.mult);
}

// hnswlib getNeighborsByHeuristic2: cand ascending by (key to the base,
// node); keeps e unless a kept r is closer to e than the base is
static inline void select_heuristic(const Graph& g,
                                    const std::vector<uint64_t>& cand,
                                    int32_t cap, std::vector<uint64_t>& out) {
  out.clear();
  if ((int32_t)cand.size() < cap) {
    out = cand;
    return;
  }
  for (uint64_t e : cand) {
    if ((int32_t)out.size() >= cap) break;
    const float de = key_of(e);
    bool keep = true;
    for (uint64_t r : out)
      if (key_rows(g.metric, g.row(node_of(r)), g.row(node_of(e)), g.d) <
          de) {
        keep = false;
        break;
      }
    if (keep) out.push_back(e);
  }
}

// Appends one node (x already normalised for cosine) and links it.  One
// thread only: the graph is a function of (rows, ids order, seed).
static inline int64_t insert(Graph& g, int64_t id, const float* x,
                             Visited& vis) {
  const int64_t node = g.n;
  const int32_t level = draw_level(g, node);
  g.rows.insert(g.rows.end(), x, x + g.d);
  g.ids.push_back(id);
  g.deleted.push_back(0);
  g.levels.push_back(level);
  g.cnt0.push_back(0);
  g.links0.resize(g.links0.size() + g.maxM0, 0);
  g.up_off.push_back(g.up_off.back() + level);
  g.up_cnt.resize(g.up_cnt.size() + level, 0);
  g.up_links.resize(g.up_links.size() + (size_t)level * g.maxM, 0);
  g.n++;
  if (g.entry < 0) {
    g.entry = node;
    g.max_level = level;
    return node;
  }
  const float* q = g.row(node);
  const uint64_t ep0 =
      pack(key_rows(g.metric, q, g.row(g.entry), g.d), (uint32_t)g.entry);
  uint64_t cur = ep0;
  for (int32_t l = g.max_level; l > level; l--)
    cur = greedy(g, q, cur, l, nullptr);
  std::vector<uint64_t> W, sel, cand;
  for (int32_t l = std::min(level, g.max_level); l >= 0; l--) {
    beam(g, q, cur, l, g.ef_construction, nullptr, vis, W, nullptr);
    // hnswlib: a deleted entry point is still offered as a neighbour, so a
    // graph whose nodes are all deleted stays connected
    if (g.deleted[g.entry] && g.levels[g.entry] >= l &&
        std::find(W.begin(), W.end(), ep0) == W.end()) {
      sorted_insert(W, ep0);
      if ((int32_t)W.size() > g.ef_construction) W.pop_back();
    }
    select_heuristic(g, W, g.M, sel);
    int32_t* nc = g.cnt(node, l);
    uint32_t* nl = g.links(node, l);
    *nc = (int32_t)sel.size();
    for (size_t t = 0; t < sel.size(); t++) nl[t] = node_of(sel[t]);
    for (uint64_t s : sel) {
      const uint32_t o = node_of(s);
      int32_t* oc = g.cnt(o, l);
      uint32_t* ol = g.links(o, l);
      const int32_t ocap = g.cap(l);
      if (*oc < ocap) {
        ol[(*oc)++] = (uint32_t)node;
        continue;
      }
      cand.clear();
      cand.push_back(pack(key_of(s), (uint32_t)node));
      for (int32_t t = 0; t < *oc; t++)
        cand.push_back(
            pack(key_rows(g.metric, g.row(o), g.row(ol[t]), g.d), ol[t]));
      std::sort(cand.begin(), cand.end());
      std::vector<uint64_t> kept;
      select_heuristic(g, cand, ocap, kept);
      *oc = (int32_t)kept.size();
      for (size_t t = 0; t < kept.size(); t++) ol[t] = node_of(kept[t]);
    }
    if (!sel.empty()) cur = sel[0];
  }
  if (level > g.max_level) {
    g.entry = node;
    g.max_level = level;
  }
  return node;
}

// ---- structural check: what the container reader requires of a graph ----
static inline bool check_structure(const Graph& g, std::string& err) {
  auto fail = [&](const std::string& m) {
    err = m;
    return false;
  };
  const int64_t n = g.n;
  if ((int64_t)g.ids.size() != n || (int64_t)g.levels.size() != n ||
      (int64_t)g.deleted.size() != n || (int64_t)g.cnt0.size() != n ||
      (int64_t)g.up_off.size() != n + 1 ||
      (int64_t)g.links0.size() != n * g.maxM0 ||
      (int64_t)g.rows.size() != n * g.d)
    return fail("array sizes do not match n");
  if (n == 0)
    return g.entry == -1 && g.max_level == -1
               ? true
               : fail("an empty graph has an entry point");
  if (g.entry < 0 || g.entry >= n) return fail("entry point out of range");
  if (g.levels[g.entry] != g.max_level)
    return fail("the entry point is not on maxlevel");
  std::unordered_set<int64_t> live;
  std::vector<uint32_t> seen;
  for (int64_t i = 0; i < n; i++) {
    if (g.levels[i] < 0 || g.levels[i] > g.max_level)
      return fail("a node's level exceeds maxlevel");
    if (g.up_off[i + 1] - g.up_off[i] != g.levels[i])
      return fail("upper-level offsets do not match the levels");
    if (g.ids[i] < 0) return fail("negative label");
    if (!g.deleted[i] && !live.insert(g.ids[i]).second)
      return fail("label repeated among live nodes");
    for (int32_t j = 0; j < g.d; j++)
      if (!std::isfinite(g.row(i)[j])) return fail("non-finite row");
    for (int32_t l = 0; l <= g.levels[i]; l++) {
      const int32_t m = g.cnt(i, l);
      if (m < 0 || m > g.cap(l)) return fail("link count above its cap");
      const uint32_t* L = g.links(i, l);
      seen.assign(L, L + m);
      std::sort(seen.begin(), seen.end());
      if (std::adjacent_find(seen.begin(), seen.end()) != seen.end())
        return fail("a link repeated in one list");
      for (int32_t t = 0; t < m; t++) {
        if ((int64_t)L[t] >= n) return fail("link out of range");
        if ((int64_t)L[t] == i) return fail("link to the node itself");
        if (g.levels[L[t]] < l)
          return fail("link to a node below the list's level");
      }
    }
  }
  return true;
}

// ---- hnswlib saveIndex container (0.7.x / 0.8.x layout) ----
namespace io {
template <class T>
static inline void put(std::vector<uint8_t>& b, T v) {
  const uint8_t* p = (const uint8_t*)&v;
  b.insert(b.end(), p, p + sizeof(T));
}
struct Reader {
  const uint8_t* p;
  size_t len, pos = 0;
  bool ok = true;
  template <class T>
  T get() {
    T v{};
    if (pos + sizeof(T) > len) {
      ok = false;
      pos = len;
      return v;
    }
    memcpy(&v, p + pos, sizeof(T));
    pos += sizeof(T);
    return v;
  }
};
}  // namespace io

static inline void save(const Graph& g, std::vector<uint8_t>& b) {
  using io::put;
  b.clear();
  const uint64_t size_links0 = 4 + 4 * (uint64_t)g.maxM0;
  const uint64_t off_data = size_links0;
  const uint64_t label_off = off_data + 4 * (uint64_t)g.d;
  const uint64_t per_elem = label_off + 8;
  b.reserve(96 + (size_t)g.n * (per_elem + 4) +
            g.up_cnt.size() * (4 + 4 * (size_t)g.maxM));
  put<uint64_t>(b, 0);  // offsetLevel0
  put<uint64_t>(b, (uint64_t)std::max(g.max_elements, g.n));
  put<uint64_t>(b, (uint64_t)g.n);
  put<uint64_t>(b, per_elem);
  put<uint64_t>(b, label_off);
  put<uint64_t>(b, off_data);
  put<int32_t>(b, g.max_level);
  put<uint32_t>(b, (uint32_t)g.entry);  // -1 of an empty graph: 0xffffffff
  put<uint64_t>(b, (uint64_t)g.maxM);
  put<uint64_t>(b, (uint64_t)g.maxM0);
  put<uint64_t>(b, (uint64_t)g.M);
  put<double>(b, g.mult);
  put<uint64_t>(b, (uint64_t)g.ef_construction);
  for (int64_t i = 0; i < g.n; i++) {
    put<uint32_t>(b, (uint32_t)g.cnt0[i] | (g.deleted[i] ? 1u << 16 : 0u));
    const uint8_t* l = (const uint8_t*)&g.links0[i * g.maxM0];
    b.insert(b.end(), l, l + 4 * (size_t)g.maxM0);
    const uint8_t* r = (const uint8_t*)g.row(i);
    b.insert(b.end(), r, r + 4 * (size_t)g.d);
    put<int64_t>(b, g.ids[i]);
  }
  for (int64_t i = 0; i < g.n; i++) {
    put<uint32_t>(b, (uint32_t)g.levels[i] * (4 + 4 * (uint32_t)g.maxM));
    for (int32_t l = 1; l <= g.levels[i]; l++) {
      put<uint32_t>(b, (uint32_t)g.cnt(i, l));
      const uint8_t* p = (const uint8_t*)g.links(i, l);
      b.insert(b.end(), p, p + 4 * (size_t)g.maxM);
    }
  }
}

// Reads and checks a whole file image.  The file carries neither metric nor
// d: the caller passes them.  kEio for malformed content, kNotSupport for an
// M outside kMinLinks .. kMaxLinks.
static inline int load(const uint8_t* buf, size_t len, int32_t metric,
                       int32_t d, Graph& g, std::string& err) {
  auto eio = [&](const std::string& m) {
    err = "hnswlib container: " + m;
    return (int)kEio;
  };
  io::Reader r{buf, len};
  const uint64_t off_l0 = r.get<uint64_t>();
  const uint64_t max_el = r.get<uint64_t>();
  const uint64_t n = r.get<uint64_t>();
  const uint64_t per_elem = r.get<uint64_t>();
  const uint64_t label_off = r.get<uint64_t>();
  const uint64_t off_data = r.get<uint64_t>();
  const int32_t maxlevel = r.get<int32_t>();
  const uint32_t enter = r.get<uint32_t>();
  const uint64_t maxM = r.get<uint64_t>();
  const uint64_t maxM0 = r.get<uint64_t>();
  const uint64_t M = r.get<uint64_t>();
  const double mult = r.get<double>();
  const uint64_t efc = r.get<uint64_t>();
  if (!r.ok) return eio("truncated header");
  if (M < (uint64_t)kMinLinks || M > (uint64_t)kMaxLinks) {
    err = "hnswlib container: M = " + std::to_string(M) +
          " outside 2 .. 128";
    return (int)kNotSupport;
  }
  if (maxM != M || maxM0 != 2 * M) return eio("maxM / maxM0 do not follow M");
  if (off_l0 != 0) return eio("offsetLevel0 != 0");
  if (off_data != 4 + 4 * maxM0) return eio("offsetData != 4 + 4 * maxM0");
  if (label_off < off_data || (label_off - off_data) % 4 != 0 ||
      (label_off - off_data) / 4 != (uint64_t)d)
    return eio("the row size does not match d = " + std::to_string(d));
  if (per_elem != label_off + 8) return eio("size_data_per_element");
  if (n > max_el) return eio("cur_element_count above max_elements");
  if (n > 0xfffffffeull) return eio("too many elements");
  if (efc < 1 || efc > (uint64_t)kMaxEfConstruction || !(mult > 0.0) ||
      !std::isfinite(mult))
    return eio("ef_construction or mult out of range");
  if (len - r.pos < n * per_elem || (len - r.pos - n * per_elem) < n * 4)
    return eio("file shorter than its element count");
  Graph t;
  t.configure(d, metric, (int32_t)M, (int32_t)efc, g.seed);
  t.mult = mult;
  t.max_elements = (int64_t)max_el;
  t.n = (int64_t)n;
  t.max_level = maxlevel;
  t.entry = n == 0 ? -1 : (int64_t)enter;
  if (n == 0 && (maxlevel != -1 || enter != 0xffffffffu))
    return eio("an empty index with an entry point");
  t.rows.resize(n * d);
  t.ids.resize(n);
  t.deleted.resize(n);
  t.levels.resize(n);
  t.cnt0.resize(n);
  t.links0.resize(n * maxM0);
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t h = r.get<uint32_t>();
    if (h >> 24 || (h >> 16 & 0xfe)) return eio("unknown list header bits");
    t.cnt0[i] = (int32_t)(h & 0xffff);
    t.deleted[i] = (h >> 16) & 1;
    t.n_deleted += t.deleted[i];
    memcpy(&t.links0[i * maxM0], buf + r.pos, 4 * maxM0);
    r.pos += 4 * maxM0;
    memcpy(&t.rows[i * d], buf + r.pos, 4 * (size_t)d);
    r.pos += 4 * (size_t)d;
    t.ids[i] = r.get<int64_t>();
  }
  const uint64_t per_list = 4 + 4 * maxM;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t sz = r.get<uint32_t>();
    if (!r.ok) return eio("truncated link lists");
    if (sz % per_list != 0) return eio("linkListSize not a whole list count");
    const uint64_t lv = sz / per_list;
    if (lv > 64 || len - r.pos < sz) return eio("link lists overrun the file");
    t.levels[i] = (int32_t)lv;
    t.up_off.push_back(t.up_off.back() + (int64_t)lv);
    for (uint64_t l = 0; l < lv; l++) {
      const uint32_t h = r.get<uint32_t>();
      if (h >> 16) return eio("unknown list header bits");
      t.up_cnt.push_back((int32_t)(h & 0xffff));
      const size_t at = t.up_links.size();
      t.up_links.resize(at + maxM);
      memcpy(&t.up_links[at], buf + r.pos, 4 * maxM);
      r.pos += 4 * maxM;
    }
  }
  if (!r.ok || r.pos != len) return eio("file length is not exact");
  std::string why;
  if (!check_structure(t, why)) return eio(why);
  g = std::move(t);
  return (int)kOk;
}

}  // namespace dg_hnsw
