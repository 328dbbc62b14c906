// faiss_io.cpp — faiss-1.7.x-compatible index containers (SURVEY.md §8f
// rank 1).  The reference's snapshot/install cycle ships faiss::write_index
// files (src/vector/vector_index_snapshot_manager.cc:583-599); a drop-in
// Index role must interchange snapshots with CPU nodes, so this file
// implements the published faiss container byte layout for exactly the
// three index shapes the reference constructs:
//   FLAT     IndexIDMap2{IndexFlatL2|IndexFlatIP}  (vector_index_flat.cc:81-98)
//   IVF_FLAT IndexIVFFlat                          (vector_index_ivf_flat.cc:805-823)
//   IVF_PQ   IndexIVFPQ (by_residual, nbits 8|4)    (vector_index_raw_ivf_pq.cc:551-570)
//
// Layout (faiss 1.7.x index_write.cpp / index_read.cpp, restated from the
// published format — the reference's faiss fork is >= 1.7.3 since it uses
// faiss::SearchParameters at vector_index_flat.cc:232):
//   write_index_header: d:i32, ntotal:i64, dummy:i64=1<<20 (x2),
//                       is_trained:u8, metric:i32 (+metric_arg:f32 iff >1)
//   vector<T>:          count:u64 (elements), raw data
//   IndexFlat payload:  "xb vector" — count:u64 in FLOATS (codes bytes / 4),
//                       then ntotal*d fp32 (legacy-compatible encoding)
//   IndexIDMap2:        "IxM2" hdr, inner index, id_map as vector<i64>
//   IndexIVF header:    index header, nlist:u64, nprobe:u64, quantizer
//                       (IndexFlat holding centroids), direct_map
//                       (type:u8=0 NoMap + empty vector)
//   InvertedLists:      "ilar", nlist:u64, code_size:u64, "full",
//                       sizes vector<u64>, then per nonempty list:
//                       codes (n*code_size bytes) then ids (n x i64)
//   IndexIVFPQ:         "IwPQ", ivf header, by_residual:u8(bool),
//                       code_size:u64, PQ {d:u64, M:u64, nbits:u64,
//                       centroids vector<f32>}, inverted lists
// All integers little-endian, no alignment padding (faiss fwrite layout).
// Cosine indexes are written as IP over stored normalized vectors, exactly
// like the reference (vector_index_flat.cc:88-91).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "dg_internal.h"

namespace {

constexpr uint32_t fcc(const char s[5]) {
  return (uint32_t)(uint8_t)s[0] | ((uint32_t)(uint8_t)s[1] << 8) |
         ((uint32_t)(uint8_t)s[2] << 16) | ((uint32_t)(uint8_t)s[3] << 24);
}

struct FWriter {
  FILE* f = nullptr;
  bool ok = true;
  void raw(const void* p, size_t n) {
    if (ok && fwrite(p, 1, n, f) != n) ok = false;
  }
  void u8(uint8_t v) { raw(&v, 1); }
  void i32(int32_t v) { raw(&v, 4); }
  void u32(uint32_t v) { raw(&v, 4); }
  void i64(int64_t v) { raw(&v, 8); }
  void u64(uint64_t v) { raw(&v, 8); }
};

struct FReader {
  FILE* f = nullptr;
  bool ok = true;
  // bytes not yet consumed; ~0 = unknown (no bound applied)
  uint64_t left = ~(uint64_t)0;
  void raw(void* p, size_t n) {
    if (ok && fread(p, 1, n, f) != n) ok = false;
    if (left != ~(uint64_t)0) left = n <= left ? left - n : 0;
  }
  // learn the file size so that counts read from the file can be bounded
  // by the bytes that are actually there before anything is resized
  void measure() {
    long pos = ftell(f);
    if (pos < 0 || fseek(f, 0, SEEK_END) != 0) return;
    long end = ftell(f);
    if (end >= pos) left = (uint64_t)(end - pos);
    fseek(f, pos, SEEK_SET);
  }
  // count elements of elem bytes each still fit in the file
  bool fits(uint64_t count, uint64_t elem) const {
    return ok && (elem == 0 || count <= left / elem);
  }
  uint8_t u8() { uint8_t v = 0; raw(&v, 1); return v; }
  int32_t i32() { int32_t v = 0; raw(&v, 4); return v; }
  uint32_t u32() { uint32_t v = 0; raw(&v, 4); return v; }
  int64_t i64() { int64_t v = 0; raw(&v, 8); return v; }
  uint64_t u64() { uint64_t v = 0; raw(&v, 8); return v; }
};

// faiss MetricType: 0 = INNER_PRODUCT, 1 = L2
int to_faiss_metric(int32_t m) { return m == DG_METRIC_L2 ? 1 : 0; }

void write_index_header(FWriter& w, int32_t d, int64_t ntotal, bool trained,
                        int faiss_metric) {
  w.i32(d);
  w.i64(ntotal);
  w.i64(1 << 20);  // dummy (faiss legacy fields)
  w.i64(1 << 20);
  w.u8(trained ? 1 : 0);
  w.i32(faiss_metric);
  // metric_arg written only for metric > 1 (never for L2/IP)
}

struct IdxHeader {
  int32_t d;
  int64_t ntotal;
  bool trained;
  int32_t metric;  // faiss metric
};

bool read_index_header(FReader& r, IdxHeader& h) {
  h.d = r.i32();
  h.ntotal = r.i64();
  (void)r.i64();
  (void)r.i64();
  h.trained = r.u8() != 0;
  h.metric = r.i32();
  if (h.metric > 1) (void)r.u32();  // metric_arg (f32)
  return r.ok && h.d > 0 && h.ntotal >= 0;
}

// IndexFlat payload: xb-vector encoding (count in floats, data = raw fp32)
void write_flat_index(FWriter& w, int32_t d, int64_t n, int faiss_metric,
                      const float* data) {
  w.u32(faiss_metric == 1 ? fcc("IxF2") : fcc("IxFI"));
  write_index_header(w, d, n, true, faiss_metric);
  w.u64((uint64_t)n * d);  // count in floats
  w.raw(data, (size_t)n * d * 4);
}

bool read_flat_index(FReader& r, IdxHeader& h, std::vector<float>& data) {
  uint32_t h4 = r.u32();
  if (h4 != fcc("IxF2") && h4 != fcc("IxFI")) return false;
  if (!read_index_header(r, h)) return false;
  h.metric = (h4 == fcc("IxF2")) ? 1 : 0;
  uint64_t count = r.u64();
  if (!r.ok || count != (uint64_t)h.ntotal * h.d) return false;
  data.resize(count);
  r.raw(data.data(), count * 4);
  return r.ok;
}

void write_direct_map(FWriter& w) {
  w.u8(0);   // DirectMap::NoMap
  w.u64(0);  // empty array
}

bool read_direct_map(FReader& r) {
  uint8_t type = r.u8();
  uint64_t n = r.u64();
  if (!r.fits(n, 8)) return false;
  if (type == 0 || type == 1) {
    // NoMap stores an empty array; Array stores ntotal entries
    std::vector<int64_t> skip(n);
    if (n) r.raw(skip.data(), n * 8);
    return r.ok;
  }
  if (type == 2) {  // Hashtable: vector of (key,id) pairs
    std::vector<int64_t> skip(n);
    if (n) r.raw(skip.data(), n * 8);
    return r.ok;
  }
  return false;
}

// host copies of the index data needed for writing
struct HostRows {
  std::vector<float> vectors;   // arrival order (FLAT/IVF)
  std::vector<uint8_t> codes;   // arrival order (PQ)
  std::vector<int64_t> ids;     // arrival order, -2 = tombstone
  std::vector<int32_t> assign;  // arrival order
};

dg_status download_rows(dg_index* ix, HostRows& h) {
  const int64_t n = ix->ntotal;
  const int32_t du = ix->d_user;   // file stride = caller's dimension
  const int32_t dp = ix->desc.d;   // device stride (padded)
  const bool is_pq = ix->desc.kind == DG_INDEX_IVF_PQ;
  h.ids.resize(n);
  h.assign.resize(n);
  if (n == 0) return DG_OK;
  if (hipMemcpy(h.ids.data(), ix->d_ids.p, (size_t)n * 8,
                hipMemcpyDeviceToHost) != hipSuccess)
    return DG_EINTERNAL;
  if (hipMemcpy(h.assign.data(), ix->d_assign.p, (size_t)n * 4,
                hipMemcpyDeviceToHost) != hipSuccess)
    return DG_EINTERNAL;
  if (is_pq) {
    h.codes.resize((size_t)n * dg_pq_code_size(ix->desc));
    if (hipMemcpy(h.codes.data(), ix->d_codes.p, h.codes.size(),
                  hipMemcpyDeviceToHost) != hipSuccess)
      return DG_EINTERNAL;
  } else {
    h.vectors.resize((size_t)n * du);
    if (hipMemcpy2D(h.vectors.data(), (size_t)du * 4, ix->d_vectors.p,
                    (size_t)dp * 4, (size_t)du * 4, (size_t)n,
                    hipMemcpyDeviceToHost) != hipSuccess)
      return DG_EINTERNAL;
  }
  return DG_OK;
}

// group kept (non-tombstoned) rows by list: returns per-list row indexes
void group_rows(const HostRows& h, int32_t nlist,
                std::vector<std::vector<int64_t>>& lists, int64_t* kept) {
  lists.assign(nlist, {});
  int64_t k = 0;
  for (int64_t i = 0; i < (int64_t)h.ids.size(); i++) {
    if (h.ids[i] < 0) continue;  // tombstone
    int32_t l = h.assign[i];
    if (l >= 0 && l < nlist) {
      lists[l].push_back(i);
      k++;
    }
  }
  *kept = k;
}

void write_invlists(FWriter& w, const HostRows& h,
                    const std::vector<std::vector<int64_t>>& lists,
                    size_t code_size, int32_t d, bool is_pq, int32_t M) {
  w.u32(fcc("ilar"));
  w.u64(lists.size());
  w.u64(code_size);
  w.u32(fcc("full"));
  w.u64(lists.size());  // sizes vector count
  for (auto& l : lists) w.u64(l.size());
  std::vector<uint8_t> cbuf;
  std::vector<int64_t> ibuf;
  for (auto& l : lists) {
    if (l.empty()) continue;
    cbuf.resize(l.size() * code_size);
    ibuf.resize(l.size());
    for (size_t j = 0; j < l.size(); j++) {
      int64_t row = l[j];
      if (is_pq)
        memcpy(cbuf.data() + j * code_size, h.codes.data() + row * M,
               code_size);
      else
        memcpy(cbuf.data() + j * code_size,
               h.vectors.data() + (size_t)row * d, code_size);
      ibuf[j] = h.ids[row];
    }
    w.raw(cbuf.data(), cbuf.size());
    w.raw(ibuf.data(), ibuf.size() * 8);
  }
}

struct InvLists {
  uint64_t nlist = 0, code_size = 0;
  std::vector<std::vector<uint8_t>> codes;
  std::vector<std::vector<int64_t>> ids;
};

// want_nlist: the nlist the index header stated.  Everything below is
// sized by it, so it has to match before anything is allocated.
bool read_invlists(FReader& r, InvLists& il, uint64_t want_nlist) {
  if (r.u32() != fcc("ilar")) return false;
  il.nlist = r.u64();
  il.code_size = r.u64();
  if (!r.ok || il.nlist != want_nlist || il.nlist > (1u << 24) ||
      il.code_size > (1u << 20))
    return false;
  uint32_t lt = r.u32();
  std::vector<uint64_t> sizes(il.nlist, 0);
  if (lt == fcc("full")) {
    uint64_t cnt = r.u64();
    if (cnt != il.nlist || !r.fits(cnt, 8)) return false;
    r.raw(sizes.data(), il.nlist * 8);
  } else if (lt == fcc("sprs")) {
    uint64_t cnt = r.u64();  // count of u64s: pairs of (idx, size)
    if (!r.fits(cnt, 8)) return false;
    std::vector<uint64_t> pairs(cnt);
    r.raw(pairs.data(), cnt * 8);
    for (uint64_t j = 0; j + 1 < cnt; j += 2) {
      if (pairs[j] >= il.nlist) return false;
      sizes[pairs[j]] = pairs[j + 1];
    }
  } else {
    return false;
  }
  if (!r.ok) return false;
  il.codes.resize(il.nlist);
  il.ids.resize(il.nlist);
  for (uint64_t l = 0; l < il.nlist; l++) {
    uint64_t n = sizes[l];
    if (!n) continue;
    if (!r.fits(n, il.code_size + 8)) return false;
    il.codes[l].resize(n * il.code_size);
    il.ids[l].resize(n);
    r.raw(il.codes[l].data(), il.codes[l].size());
    r.raw(il.ids[l].data(), n * 8);
    if (!r.ok) return false;
  }
  return true;
}

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

}  // namespace

extern "C" dg_status dg_save_faiss(dg_index* ix, const char* path) {
  if (!ix || !path) return DG_EINVAL;
  if (ix->is_bin) {
    dg_set_error("dg_save_faiss called on a binary index: use "
                 "dg_save_faiss_binary");
    return DG_ENOT_SUPPORT;
  }
  if (dg_kind_is_hnsw(ix->desc.kind)) {
    dg_set_error("dg_save_faiss called on an HNSW index: use "
                 "dg_save_hnswlib");
    return DG_ENOT_SUPPORT;
  }
  std::shared_lock lk(ix->rw);
  if (ix->storage != DG_STORAGE_F32) {
    dg_set_error("dg_save_faiss: f16 or SQ8 row storage would need a scalar-"
                 "quantiser file, which the CPU nodes' IndexIVFFlat loader "
                 "cannot read: use dg_save");
    return DG_ENOT_SUPPORT;
  }
  DeviceGuard g{ix->device};
  const int32_t d = ix->d_user;  // containers speak the caller's dimension
  const int fm = to_faiss_metric(ix->desc.metric);
  const bool is_pq = ix->desc.kind == DG_INDEX_IVF_PQ;
  const bool is_flat = ix->desc.kind == DG_INDEX_FLAT;
  if (!is_flat && !ix->trained) {
    dg_set_error("faiss save of untrained IVF index unsupported");
    return DG_ENOT_SUPPORT;
  }
  HostRows h;
  dg_status st = download_rows(ix, h);
  if (st != DG_OK) return st;

  FILE* f = fopen(path, "wb");
  if (!f) {
    dg_set_error("cannot open %s", path);
    return DG_EIO;
  }
  FWriter w{f};
  if (is_flat) {
    // IndexIDMap2 { IndexFlat }: inner codes = kept vectors in arrival
    // order; id_map = their ids (vector_index_flat.cc:81-98)
    std::vector<float> kept;
    std::vector<int64_t> idmap;
    kept.reserve(h.vectors.size());
    for (int64_t i = 0; i < ix->ntotal; i++) {
      if (h.ids[i] < 0) continue;
      kept.insert(kept.end(), h.vectors.begin() + (size_t)i * d,
                  h.vectors.begin() + (size_t)(i + 1) * d);
      idmap.push_back(h.ids[i]);
    }
    const int64_t n = (int64_t)idmap.size();
    w.u32(fcc("IxM2"));
    write_index_header(w, d, n, true, fm);
    write_flat_index(w, d, n, fm, kept.data());
    w.u64((uint64_t)n);  // id_map vector
    w.raw(idmap.data(), (size_t)n * 8);
  } else {
    const int32_t nlist = ix->desc.nlist;
    std::vector<float> cents((size_t)nlist * d);
    if (hipMemcpy2D(cents.data(), (size_t)d * 4, ix->d_centroids.p,
                    (size_t)ix->desc.d * 4, (size_t)d * 4, (size_t)nlist,
                    hipMemcpyDeviceToHost) != hipSuccess) {
      fclose(f);
      return DG_EINTERNAL;
    }
    std::vector<std::vector<int64_t>> lists;
    int64_t kept = 0;
    group_rows(h, nlist, lists, &kept);
    w.u32(is_pq ? fcc("IwPQ") : fcc("IwFl"));
    // ivf header: index header, nlist, nprobe, quantizer, direct map
    write_index_header(w, d, kept, ix->trained, fm);
    w.u64((uint64_t)nlist);
    w.u64(1);  // nprobe member default (searches pass IVFSearchParameters)
    write_flat_index(w, d, nlist, fm, cents.data());
    write_direct_map(w);
    if (is_pq) {
      const int32_t M = ix->desc.pq_m;
      const int32_t dsub = d / M;
      const int32_t nbits = ix->desc.pq_nbits;
      const int32_t cs = dg_pq_code_size(ix->desc);
      std::vector<float> cb((size_t)M * dg_pq_ksub(ix->desc) * dsub);
      if (hipMemcpy(cb.data(), ix->d_codebooks.p, cb.size() * 4,
                    hipMemcpyDeviceToHost) != hipSuccess) {
        fclose(f);
        return DG_EINTERNAL;
      }
      w.u8(1);          // by_residual (bool; faiss >= 1.7 writes 1 byte)
      w.u64((uint64_t)cs);  // code_size = M * nbits / 8 (the device layout
                            // is faiss's packing, so rows copy as they are)
      w.u64((uint64_t)d);  // ProductQuantizer.d
      w.u64((uint64_t)M);  // .M
      w.u64((uint64_t)nbits);  // .nbits
      w.u64(cb.size());    // centroids vector<float>
      w.raw(cb.data(), cb.size() * 4);
      write_invlists(w, h, lists, cs, d, true, cs);
    } else {
      write_invlists(w, h, lists, (size_t)d * 4, d, false, 0);
    }
  }
  bool ok = w.ok && fclose(f) == 0;
  if (!ok) {
    dg_set_error("write failed for %s", path);
    return DG_EIO;
  }
  return DG_OK;
}

static dg_status load_faiss_impl(dg_index** out, const char* path,
                                 int32_t metric_override, int32_t device);

extern "C" dg_status dg_load_faiss(dg_index** out, const char* path,
                                   int32_t metric_override, int32_t device) {
  // exception wall: a malformed container can drive a vector resize into
  // std::bad_alloc; no exception may cross the C ABI
  try {
    return load_faiss_impl(out, path, metric_override, device);
  } catch (const std::exception& e) {
    dg_set_error("faiss container load failed: %s", e.what());
    return DG_EIO;
  } catch (...) {
    dg_set_error("faiss container load failed");
    return DG_EIO;
  }
}

static dg_status load_faiss_impl(dg_index** out, const char* path,
                                 int32_t metric_override, int32_t device) {
  if (!out || !path) return DG_EINVAL;
  FILE* f = fopen(path, "rb");
  if (!f) {
    dg_set_error("cannot open %s", path);
    return DG_EIO;
  }
  FReader r{f};
  dg_status st = DG_EIO;
  dg_index* ix = nullptr;
  do {
    uint32_t h4 = r.u32();
    if (!r.ok) break;
    if (h4 == fcc("IxM2") || h4 == fcc("IxMp")) {
      // FLAT: IDMap(2) over IndexFlat
      IdxHeader oh;
      if (!read_index_header(r, oh)) break;
      IdxHeader ih;
      std::vector<float> data;
      if (!read_flat_index(r, ih, data)) break;
      uint64_t nmap = r.u64();
      if (!r.ok || (int64_t)nmap != ih.ntotal) break;
      std::vector<int64_t> idmap(nmap);
      if (nmap) r.raw(idmap.data(), nmap * 8);
      if (!r.ok) break;
      int32_t metric = metric_override >= 0
                           ? metric_override
                           : (ih.metric == 1 ? DG_METRIC_L2 : DG_METRIC_IP);
      if ((ih.metric == 1) != (metric == DG_METRIC_L2)) {
        dg_set_error("metric override incompatible with file metric");
        st = DG_EINVAL;
        break;
      }
      dg_index_desc desc{};
      desc.kind = DG_INDEX_FLAT;
      desc.metric = metric;
      desc.d = ih.d;
      desc.device = device;
      desc.reserve = ih.ntotal;
      if ((st = dg_index_create(&ix, &desc)) != DG_OK) break;
      st = nmap ? dg_ingest_rows(ix, nmap, idmap.data(), data.data(),
                                 nullptr, nullptr)
                : DG_OK;
    } else if (h4 == fcc("IwFl") || h4 == fcc("IwPQ")) {
      IdxHeader oh;
      if (!read_index_header(r, oh)) break;
      uint64_t nlist = r.u64();
      (void)r.u64();  // nprobe member (per-search in the reference)
      IdxHeader qh;
      std::vector<float> cents;
      if (!read_flat_index(r, qh, cents)) break;
      if ((uint64_t)qh.ntotal != nlist || qh.d != oh.d) break;
      if (!read_direct_map(r)) break;
      int32_t metric = metric_override >= 0
                           ? metric_override
                           : (oh.metric == 1 ? DG_METRIC_L2 : DG_METRIC_IP);
      if ((oh.metric == 1) != (metric == DG_METRIC_L2)) {
        dg_set_error("metric override incompatible with file metric");
        st = DG_EINVAL;
        break;
      }
      dg_index_desc desc{};
      desc.metric = metric;
      desc.d = oh.d;
      desc.nlist = (int32_t)nlist;
      desc.device = device;
      desc.reserve = oh.ntotal;
      std::vector<float> cb;
      int32_t M = 0;
      if (h4 == fcc("IwPQ")) {
        desc.kind = DG_INDEX_IVF_PQ;
        uint8_t by_residual = r.u8();
        uint64_t code_size = r.u64();
        if (!by_residual) {
          // non-residual IVFPQ files would decode with the wrong ADC
          dg_set_error("IwPQ with by_residual=0 unsupported");
          st = DG_ENOT_SUPPORT;
          break;
        }
        uint64_t pq_d = r.u64();
        uint64_t pq_M = r.u64();
        uint64_t pq_nbits = r.u64();
        if (!r.ok || (pq_nbits != 8 && pq_nbits != 4) ||
            pq_d != (uint64_t)oh.d || pq_M == 0 || pq_M > (uint64_t)oh.d ||
            pq_M * pq_nbits != code_size * 8 || oh.d % pq_M != 0) {
          dg_set_error(
              "unsupported IwPQ parameters (code_size=%llu M=%llu nbits=%llu"
              " — only nbits 4 or 8 with code_size = M*nbits/8 and "
              "by_residual are supported)",
              (unsigned long long)code_size, (unsigned long long)pq_M,
              (unsigned long long)pq_nbits);
          st = DG_ENOT_SUPPORT;
          break;
        }
        M = (int32_t)pq_M;
        desc.pq_m = M;
        desc.pq_nbits = (int32_t)pq_nbits;
        uint64_t nc = r.u64();
        if (!r.ok || nc != ((uint64_t)M << pq_nbits) * (oh.d / M)) break;
        cb.resize(nc);
        r.raw(cb.data(), nc * 4);
        if (!r.ok) break;
      } else {
        desc.kind = DG_INDEX_IVF_FLAT;
      }
      InvLists il;
      if (!read_invlists(r, il, nlist)) break;
      size_t want_cs = h4 == fcc("IwPQ") ? (size_t)dg_pq_code_size(desc)
                                         : (size_t)oh.d * 4;
      if (il.code_size != want_cs) break;
      if ((st = dg_index_create(&ix, &desc)) != DG_OK) break;
      if ((st = dg_set_centroids(ix, (int32_t)nlist, cents.data())) != DG_OK)
        break;
      if (h4 == fcc("IwPQ") &&
          (st = dg_set_codebooks(ix, M, desc.pq_nbits, cb.data())) != DG_OK)
        break;
      // flatten lists into arrival arrays with their file assignment
      std::vector<int64_t> ids;
      std::vector<int32_t> assign;
      std::vector<float> vecs;
      std::vector<uint8_t> codes;
      for (uint64_t l = 0; l < nlist; l++) {
        size_t n = il.ids[l].size();
        if (!n) continue;
        ids.insert(ids.end(), il.ids[l].begin(), il.ids[l].end());
        assign.insert(assign.end(), n, (int32_t)l);
        if (h4 == fcc("IwPQ"))
          codes.insert(codes.end(), il.codes[l].begin(), il.codes[l].end());
        else {
          const float* v = (const float*)il.codes[l].data();
          vecs.insert(vecs.end(), v, v + n * oh.d);
        }
      }
      st = ids.empty()
               ? DG_OK
               : dg_ingest_rows(ix, (int64_t)ids.size(), ids.data(),
                                vecs.empty() ? nullptr : vecs.data(),
                                codes.empty() ? nullptr : codes.data(),
                                assign.data());
    } else {
      dg_set_error("unsupported faiss index fourcc 0x%08x", h4);
      st = DG_ENOT_SUPPORT;
    }
  } while (0);
  fclose(f);
  if (st != DG_OK) {
    if (ix) dg_index_destroy(ix);
    if (st == DG_EIO) dg_set_error("malformed faiss container %s", path);
    return st;
  }
  *out = ix;
  return DG_OK;
}

// ---------------- binary (Hamming) containers ----------------
// faiss 1.7.x write_index_binary layout for the two shapes the reference
// constructs over faiss::IndexBinary (vector_index_flat.cc:99-102,
// vector_index_ivf_flat.cc:75-80):
//   binary header: d:i32, code_size:i32 (= d/8), ntotal:i64, is_trained:u8,
//                  metric_type:i32 (= 1) — 21 bytes, no dummy fields
//   IndexBinaryFlat    "IBxF" header, xb vector<u8> (ntotal * code_size)
//   IndexBinaryIDMap2  "IBM2" ("IBMp" = IDMap) header, inner index, id_map
//   IndexBinaryIVF     "IBwF" header, nlist:u64, nprobe:u64, quantizer
//                      (IBxF holding the centroids), direct map, inverted
//                      lists as in the float IVF ("ilar", code_size = d/8)
namespace {

constexpr int32_t kBinMaxNlist = 1023 * 256 - 1;  // scan-length cap, dg_abi

void write_binary_header(FWriter& w, int32_t d, int64_t ntotal, bool trained) {
  w.i32(d);
  w.i32(d / 8);
  w.i64(ntotal);
  w.u8(trained ? 1 : 0);
  w.i32(1);  // METRIC_L2: what faiss::IndexBinary carries
}

void write_binary_flat(FWriter& w, int32_t d, int64_t n, const uint8_t* xb) {
  w.u32(fcc("IBxF"));
  write_binary_header(w, d, n, true);
  w.u64((uint64_t)n * (d / 8));
  if (n) w.raw(xb, (size_t)n * (d / 8));
}

struct BinHeader {
  int32_t d = 0, code_size = 0, metric = 0;
  int64_t ntotal = 0;
  bool trained = false;
};

// DG_OK, DG_EIO (malformed) or DG_ENOT_SUPPORT (a metric other than L2,
// which the reference rejects too, vector_index_flat.cc:433-438, or an
// untrained index)
dg_status read_binary_header(FReader& r, BinHeader& h) {
  h.d = r.i32();
  h.code_size = r.i32();
  h.ntotal = r.i64();
  h.trained = r.u8() != 0;
  h.metric = r.i32();
  if (!r.ok) return DG_EIO;
  if (h.d < 8 || h.d > 32768 || h.d % 8 != 0 || h.code_size != h.d / 8 ||
      h.ntotal < 0)
    return DG_EIO;
  if (h.metric != 1) {
    dg_set_error("binary faiss container with metric_type %d unsupported "
                 "(only METRIC_L2 = 1)", h.metric);
    return DG_ENOT_SUPPORT;
  }
  if (!h.trained) {
    // the writer refuses an untrained index and the reference refuses to
    // load one (vector_index_flat.cc:408-410)
    dg_set_error("binary faiss container with is_trained = 0 unsupported");
    return DG_ENOT_SUPPORT;
  }
  return DG_OK;
}

dg_status unsupported_fourcc(uint32_t h4) {
  dg_set_error("unsupported binary faiss index fourcc 0x%08x '%c%c%c%c'", h4,
               (h4 & 0x7f) >= 32 ? (int)(h4 & 0x7f) : '?',
               ((h4 >> 8) & 0x7f) >= 32 ? (int)((h4 >> 8) & 0x7f) : '?',
               ((h4 >> 16) & 0x7f) >= 32 ? (int)((h4 >> 16) & 0x7f) : '?',
               ((h4 >> 24) & 0x7f) >= 32 ? (int)((h4 >> 24) & 0x7f) : '?');
  return DG_ENOT_SUPPORT;
}

// "IBxF" index whose dimension must equal d
dg_status read_binary_flat(FReader& r, int32_t d, BinHeader& h,
                           std::vector<uint8_t>& xb) {
  uint32_t h4 = r.u32();
  if (!r.ok) return DG_EIO;
  if (h4 != fcc("IBxF")) return unsupported_fourcc(h4);
  dg_status st = read_binary_header(r, h);
  if (st != DG_OK) return st;
  if (h.d != d) return DG_EIO;
  uint64_t count = r.u64();
  if (!r.ok || !r.fits(count, 1) ||
      !r.fits((uint64_t)h.ntotal, (uint64_t)h.code_size) ||
      count != (uint64_t)h.ntotal * (uint64_t)h.code_size)
    return DG_EIO;
  xb.resize(count);
  if (count) r.raw(xb.data(), count);
  return r.ok ? DG_OK : DG_EIO;
}

// negative ids are reserved (a negative stored id marks a removed row)
bool ids_valid(const std::vector<int64_t>& ids) {
  for (int64_t id : ids)
    if (id < 0) return false;
  return true;
}

// everything a binary container holds, parsed on the host
struct BinFile {
  int32_t kind = 0, d = 0, nlist = 0;
  std::vector<uint8_t> cents;   // IVF: nlist x d/8
  std::vector<int64_t> ids;     // file order
  std::vector<uint8_t> rows;    // ids.size() x d/8
  std::vector<int32_t> assign;  // IVF: list of every row
};

dg_status parse_binary(FReader& r, BinFile& bf) {
  uint32_t h4 = r.u32();
  if (!r.ok) return DG_EIO;
  dg_status st;
  if (h4 == fcc("IBM2") || h4 == fcc("IBMp")) {
    BinHeader oh, ih;
    if ((st = read_binary_header(r, oh)) != DG_OK) return st;
    if ((st = read_binary_flat(r, oh.d, ih, bf.rows)) != DG_OK) return st;
    uint64_t nmap = r.u64();
    if (!r.ok || !r.fits(nmap, 8) || nmap != (uint64_t)ih.ntotal ||
        oh.ntotal != ih.ntotal)
      return DG_EIO;
    bf.ids.resize(nmap);
    if (nmap) r.raw(bf.ids.data(), nmap * 8);
    if (!r.ok || !ids_valid(bf.ids)) return DG_EIO;
    bf.kind = DG_INDEX_BINARY_FLAT;
    bf.d = oh.d;
    return DG_OK;
  }
  if (h4 == fcc("IBwF")) {
    BinHeader oh, qh;
    if ((st = read_binary_header(r, oh)) != DG_OK) return st;
    uint64_t nlist = r.u64();
    (void)r.u64();  // nprobe member (per-search in the reference)
    if (!r.ok || nlist == 0 || nlist > (uint64_t)kBinMaxNlist) return DG_EIO;
    if ((st = read_binary_flat(r, oh.d, qh, bf.cents)) != DG_OK) return st;
    if ((uint64_t)qh.ntotal != nlist) return DG_EIO;
    if (!read_direct_map(r)) return DG_EIO;
    InvLists il;
    if (!read_invlists(r, il, nlist)) return DG_EIO;  // nlist <= the cap
    if (il.code_size != (uint64_t)oh.code_size) return DG_EIO;
    int64_t total = 0;
    for (uint64_t l = 0; l < nlist; l++) {
      const size_t n = il.ids[l].size();
      if (!n) continue;
      total += (int64_t)n;
      bf.ids.insert(bf.ids.end(), il.ids[l].begin(), il.ids[l].end());
      bf.rows.insert(bf.rows.end(), il.codes[l].begin(), il.codes[l].end());
      bf.assign.insert(bf.assign.end(), n, (int32_t)l);
    }
    if (total != oh.ntotal || !ids_valid(bf.ids)) return DG_EIO;
    bf.kind = DG_INDEX_BINARY_IVF_FLAT;
    bf.d = oh.d;
    bf.nlist = (int32_t)nlist;
    return DG_OK;
  }
  return unsupported_fourcc(h4);
}

dg_status load_faiss_binary_impl(dg_index** out, const char* path,
                                 int32_t device) {
  if (!out || !path) return DG_EINVAL;
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) {
    dg_set_error("cannot open %s", path);
    return DG_EIO;
  }
  // the whole file is read and checked on the host before the first device
  // call: a malformed container is answered without a GPU
  BinFile bf;
  dg_status st;
  {
    FReader r{f};
    r.measure();
    try {
      st = parse_binary(r, bf);
    } catch (...) {
      fclose(f);
      throw;
    }
  }
  fclose(f);
  if (st != DG_OK) {
    if (st == DG_EIO) dg_set_error("malformed binary faiss container %s", path);
    return st;
  }
  dg_index_desc desc{};
  desc.kind = bf.kind;
  desc.metric = DG_METRIC_HAMMING;
  desc.d = bf.d;
  desc.nlist = bf.nlist;
  desc.device = device;
  desc.reserve = (int64_t)bf.ids.size();
  dg_index* ix = nullptr;
  if ((st = dg_index_create(&ix, &desc)) != DG_OK) return st;
  if (bf.kind == DG_INDEX_BINARY_IVF_FLAT)
    st = dg_set_centroids_binary(ix, bf.nlist, bf.cents.data());
  // rows keep the list the file puts them in (no re-assignment)
  if (st == DG_OK && !bf.ids.empty())
    st = dg_ingest_bits(ix, (int64_t)bf.ids.size(), bf.ids.data(),
                        bf.rows.data(),
                        bf.assign.empty() ? nullptr : bf.assign.data());
  if (st != DG_OK) {
    dg_index_destroy(ix);
    return st;
  }
  *out = ix;
  return DG_OK;
}

}  // namespace

extern "C" dg_status dg_save_faiss_binary(dg_index* ix, const char* path) {
  if (!ix || !path) return DG_EINVAL;
  if (!ix->is_bin) {
    dg_set_error("dg_save_faiss_binary called on a float index (kind %d): "
                 "use dg_save_faiss", ix->desc.kind);
    return DG_EINVAL;
  }
  std::shared_lock lk(ix->rw);
  DeviceGuard g{ix->device};
  const int32_t d = ix->d_user;
  const size_t cs = (size_t)d / 8;  // file row = d/8 bytes, word pad stripped
  const bool is_flat = ix->desc.kind == DG_INDEX_BINARY_FLAT;
  if (!is_flat && !ix->trained) {
    dg_set_error("faiss save of untrained IVF index unsupported");
    return DG_ENOT_SUPPORT;
  }
  const int64_t n = ix->ntotal;
  HostRows h;  // codes = packed rows, arrival order
  h.ids.resize(n);
  h.assign.resize(n);
  h.codes.resize((size_t)n * cs);
  if (n) {
    if (hipMemcpy(h.ids.data(), ix->d_ids.p, (size_t)n * 8,
                  hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h.assign.data(), ix->d_assign.p, (size_t)n * 4,
                  hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy2D(h.codes.data(), cs, ix->d_codes.p, (size_t)ix->b_wp * 4,
                    cs, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) {
      dg_set_error("row download failed");
      return DG_EINTERNAL;
    }
  }
  std::vector<uint8_t> cents;
  if (!is_flat) {
    cents.resize((size_t)ix->desc.nlist * cs);
    if (hipMemcpy2D(cents.data(), cs, ix->d_centroids.p, (size_t)ix->b_wp * 4,
                    cs, (size_t)ix->desc.nlist,
                    hipMemcpyDeviceToHost) != hipSuccess) {
      dg_set_error("centroid download failed");
      return DG_EINTERNAL;
    }
  }
  FILE* f = fopen(path, "wb");
  if (!f) {
    dg_set_error("cannot open %s", path);
    return DG_EIO;
  }
  FWriter w{f};
  if (is_flat) {
    // IndexBinaryIDMap2 { IndexBinaryFlat }: kept rows in arrival order
    std::vector<uint8_t> kept;
    std::vector<int64_t> idmap;
    kept.reserve(h.codes.size());
    for (int64_t i = 0; i < n; i++) {
      if (h.ids[i] < 0) continue;  // tombstone
      kept.insert(kept.end(), h.codes.begin() + (size_t)i * cs,
                  h.codes.begin() + (size_t)(i + 1) * cs);
      idmap.push_back(h.ids[i]);
    }
    const int64_t nk = (int64_t)idmap.size();
    w.u32(fcc("IBM2"));
    write_binary_header(w, d, nk, true);
    write_binary_flat(w, d, nk, kept.data());
    w.u64((uint64_t)nk);
    if (nk) w.raw(idmap.data(), (size_t)nk * 8);
  } else {
    const int32_t nlist = ix->desc.nlist;
    std::vector<std::vector<int64_t>> lists;
    int64_t kept = 0;
    group_rows(h, nlist, lists, &kept);
    w.u32(fcc("IBwF"));
    write_binary_header(w, d, kept, true);
    w.u64((uint64_t)nlist);
    w.u64(1);  // nprobe member default (searches pass their own)
    write_binary_flat(w, d, nlist, cents.data());
    write_direct_map(w);
    // rows are byte codes of cs bytes held in h.codes, which is what
    // write_invlists' "PQ" form copies: is_pq = true, M = bytes per row
    write_invlists(w, h, lists, cs, d, /*is_pq=*/true, /*M=*/(int32_t)cs);
  }
  bool ok = w.ok;
  ok = (fclose(f) == 0) && ok;
  if (!ok) {
    dg_set_error("write failed for %s", path);
    return DG_EIO;
  }
  return DG_OK;
}

extern "C" dg_status dg_load_faiss_binary(dg_index** out, const char* path,
                                          int32_t device) {
  // exception wall, as dg_load_faiss
  try {
    return load_faiss_binary_impl(out, path, device);
  } catch (const std::exception& e) {
    dg_set_error("binary faiss container load failed: %s", e.what());
    return DG_EIO;
  } catch (...) {
    dg_set_error("binary faiss container load failed");
    return DG_EIO;
  }
}
