"""dingostore — ctypes wrapper over the MI355X-native index library
(dingo-store_amd/libdingo_gpu.so).

This is the PRODUCT path: it loads the HIP library built for gfx950 and
fails loudly if the library or a GPU is missing.  There is no CPU fallback
anywhere behind these calls.
"""
import ctypes as C
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libdingo_gpu.so")

L2, IP, COSINE = 0, 1, 2
FLAT, IVF_FLAT, IVF_PQ = 0, 1, 2
# binary (Hamming) indexes: d is in bits, rows are np.uint8 [n, d // 8]
BINARY_FLAT, BINARY_IVF_FLAT = 3, 4
# graph index: host-built HNSW graph, searched by one kernel (one wave per
# query); hnsw_configure / set_ef / search_hnsw / save_hnswlib below
HNSW = 5
HAMMING = 3
# row storage of an IVF_FLAT index (dg_storage)
STORAGE_F32, STORAGE_F16, STORAGE_SQ8 = 0, 1, 2
_STORAGE = {"f32": STORAGE_F32, "f16": STORAGE_F16, "sq8": STORAGE_SQ8}


def _storage_code(storage):
    if storage not in _STORAGE:
        raise DgError(
            f"storage must be 'f32', 'f16' or 'sq8', got {storage!r}")
    return _STORAGE[storage]

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")


class DgError(RuntimeError):
    pass


class _Desc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("metric", C.c_int32), ("d", C.c_int32),
        ("nlist", C.c_int32), ("pq_m", C.c_int32), ("pq_nbits", C.c_int32),
        ("device", C.c_int32), ("reserve", C.c_int64),
    ]


class _Filter(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("negate", C.c_int32),
        ("min_id", C.c_int64), ("max_id", C.c_int64),
        ("ids", C.c_void_p), ("n_ids", C.c_int64),
        ("bitmap", C.c_void_p), ("bitmap_base", C.c_int64),
        ("bitmap_nbits", C.c_int64),
    ]


class _Stats(C.Structure):
    _fields_ = [
        ("ntotal", C.c_int64), ("d", C.c_int32), ("metric", C.c_int32),
        ("kind", C.c_int32), ("nlist", C.c_int32), ("is_trained", C.c_int32),
        ("_pad", C.c_int32), ("device_bytes", C.c_int64),
        ("last_coarse_ms", C.c_double), ("last_scan_ms", C.c_double),
        ("last_select_ms", C.c_double), ("last_total_ms", C.c_double),
        ("last_nq", C.c_int64),
        ("last_scan_bytes_algorithmic", C.c_int64),
        ("last_scan_gbps_algorithmic", C.c_double),
        ("deleted_count", C.c_int64),
    ]


class _HnswInfo(C.Structure):
    _fields_ = [
        ("nlinks", C.c_int32), ("max_m0", C.c_int32),
        ("ef_construction", C.c_int32), ("ef_search", C.c_int32),
        ("max_level", C.c_int32), ("entry_point", C.c_int64),
        ("n_nodes", C.c_int64), ("n_deleted", C.c_int64),
        ("seed", C.c_uint64),
    ]


class _BatchOpts(C.Structure):
    _fields_ = [("max_batch", C.c_int32), ("max_wait_us", C.c_int32)]


class _BatchStats(C.Structure):
    _fields_ = [
        ("calls", C.c_int64), ("queries", C.c_int64), ("flushes", C.c_int64),
        ("max_flush_queries", C.c_int64), ("bypassed", C.c_int64),
    ]


def _load():
    if not os.path.exists(_SO):
        raise DgError(
            f"{_SO} missing — build it with __graft_entry__.build() "
            "(the GPU product path has no fallback)")
    lib = C.CDLL(_SO)
    lib.dg_build_info.restype = C.c_char_p
    lib.dg_device_count.restype = C.c_int
    lib.dg_last_error.argtypes = [C.c_char_p, C.c_int64]
    lib.dg_index_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(_Desc)]
    lib.dg_index_destroy.argtypes = [C.c_void_p]
    lib.dg_train.argtypes = [C.c_void_p, C.c_int64, _f32p]
    lib.dg_set_centroids.argtypes = [C.c_void_p, C.c_int32, _f32p]
    lib.dg_get_centroids.argtypes = [C.c_void_p, _f32p]
    lib.dg_add.argtypes = [C.c_void_p, C.c_int64, _i64p, _f32p]
    lib.dg_upsert.argtypes = [C.c_void_p, C.c_int64, _i64p, _f32p]
    lib.dg_remove.argtypes = [C.c_void_p, C.c_int64, _i64p]
    lib.dg_search.argtypes = [
        C.c_void_p, C.c_int64, _f32p, C.c_int32, C.c_int32,
        C.POINTER(_Filter), _f32p, _i64p,
    ]
    lib.dg_search_device.argtypes = [
        C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
        C.POINTER(_Filter), C.c_void_p, C.c_void_p,
    ]
    lib.dg_sync.argtypes = [C.c_void_p]
    lib.dg_save.argtypes = [C.c_void_p, C.c_char_p]
    lib.dg_load.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_int32]
    lib.dg_stats.argtypes = [C.c_void_p, C.POINTER(_Stats)]
    lib.dg_set_list_mask.argtypes = [C.c_void_p, C.c_void_p]
    lib.dg_mirror_selftest.restype = C.c_int
    lib.dg_train_binary.argtypes = [C.c_void_p, C.c_int64, _u8p]
    lib.dg_set_centroids_binary.argtypes = [C.c_void_p, C.c_int32, _u8p]
    lib.dg_get_centroids_binary.argtypes = [C.c_void_p, _u8p]
    lib.dg_add_binary.argtypes = [C.c_void_p, C.c_int64, _i64p, _u8p]
    lib.dg_upsert_binary.argtypes = [C.c_void_p, C.c_int64, _i64p, _u8p]
    lib.dg_search_binary.argtypes = [
        C.c_void_p, C.c_int64, _u8p, C.c_int32, C.c_int32,
        C.POINTER(_Filter), _f32p, _i64p,
    ]
    lib.dg_search_binary_device.argtypes = [
        C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32,
        C.POINTER(_Filter), C.c_void_p, C.c_void_p,
    ]
    lib.dg_mirror_selftest_binary.restype = C.c_int
    lib.dg_mirror_selftest_pq4.restype = C.c_int
    lib.dg_range_search_binary.argtypes = [
        C.c_void_p, C.c_int64, _u8p, C.c_int32, C.c_int32,
        C.POINTER(_Filter), _i64p, C.POINTER(C.POINTER(C.c_int64)),
        C.POINTER(C.POINTER(C.c_float)),
    ]
    lib.dg_save_faiss_binary.argtypes = [C.c_void_p, C.c_char_p]
    lib.dg_load_faiss_binary.argtypes = [C.POINTER(C.c_void_p), C.c_char_p,
                                         C.c_int32]
    lib.dg_free.argtypes = [C.c_void_p]
    lib.dg_batching_enable.argtypes = [C.c_void_p, C.POINTER(_BatchOpts)]
    lib.dg_batching_disable.argtypes = [C.c_void_p]
    lib.dg_batching_stats.argtypes = [C.c_void_p, C.POINTER(_BatchStats)]
    lib.dg_search_batched.argtypes = lib.dg_search.argtypes
    lib.dg_search_binary_batched.argtypes = lib.dg_search_binary.argtypes
    lib.dg_mirror_selftest_batched.restype = C.c_int
    lib.dg_bench_threads.argtypes = [
        C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f32p, C.c_int64,
        C.c_int32, C.c_int32,
    ]
    lib.dg_bench_threads.restype = C.c_double
    # list merge and the sharded index
    lib.dg_merge_topk.argtypes = [
        C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _f32p, _i64p,
        _f32p, _i64p, C.c_int32,
    ]
    lib.dg_merge_topk_device.argtypes = [
        C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
    ]
    _i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.dg_sharded_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(_Desc),
                                      C.c_int32, _i32p]
    lib.dg_sharded_destroy.argtypes = [C.c_void_p]
    lib.dg_sharded_train.argtypes = [C.c_void_p, C.c_int64, _f32p]
    lib.dg_sharded_set_centroids.argtypes = [C.c_void_p, C.c_int32, _f32p]
    lib.dg_sharded_get_centroids.argtypes = [C.c_void_p, _f32p]
    lib.dg_sharded_set_codebooks.argtypes = [C.c_void_p, C.c_int32, C.c_int32,
                                             _f32p]
    lib.dg_sharded_get_codebooks.argtypes = [C.c_void_p, _f32p]
    lib.dg_sharded_add.argtypes = [C.c_void_p, C.c_int64, _i64p, _f32p]
    lib.dg_sharded_upsert.argtypes = [C.c_void_p, C.c_int64, _i64p, _f32p]
    lib.dg_sharded_remove.argtypes = [C.c_void_p, C.c_int64, _i64p]
    lib.dg_sharded_search.argtypes = lib.dg_search.argtypes
    lib.dg_sharded_search_device.argtypes = lib.dg_search_device.argtypes
    lib.dg_sharded_sync.argtypes = [C.c_void_p]
    lib.dg_sharded_range_search.argtypes = [
        C.c_void_p, C.c_int64, _f32p, C.c_float, C.POINTER(_Filter), _i64p,
        C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.POINTER(C.c_float)),
    ]
    lib.dg_sharded_stats.argtypes = [C.c_void_p, C.POINTER(_Stats)]
    lib.dg_sharded_n_shards.argtypes = [C.c_void_p]
    lib.dg_sharded_n_shards.restype = C.c_int32
    lib.dg_sharded_shard.argtypes = [C.c_void_p, C.c_int32]
    lib.dg_sharded_shard.restype = C.c_void_p
    lib.dg_mirror_selftest_sharded.restype = C.c_int
    # row storage and read-back
    lib.dg_set_storage.argtypes = [C.c_void_p, C.c_int32]
    lib.dg_get_storage.argtypes = [C.c_void_p]
    lib.dg_get_storage.restype = C.c_int32
    lib.dg_reconstruct.argtypes = [C.c_void_p, C.c_int64, _i64p, _f32p]
    lib.dg_last_scan_f16.argtypes = [C.c_void_p]
    lib.dg_last_scan_f16.restype = C.c_int
    lib.dg_sharded_set_storage.argtypes = [C.c_void_p, C.c_int32]
    lib.dg_mirror_selftest_f16.restype = C.c_int
    # SQ8 row storage
    lib.dg_set_sq_ranges.argtypes = [C.c_void_p, _f32p, _f32p]
    lib.dg_get_sq_ranges.argtypes = [C.c_void_p, _f32p, _f32p]
    lib.dg_last_scan_sq8.argtypes = [C.c_void_p]
    lib.dg_last_scan_sq8.restype = C.c_int
    lib.dg_sharded_set_sq_ranges.argtypes = [C.c_void_p, _f32p, _f32p]
    lib.dg_sharded_get_sq_ranges.argtypes = [C.c_void_p, _f32p, _f32p]
    lib.dg_mirror_selftest_sq8.restype = C.c_int
    # HNSW
    _u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
    lib.dg_hnsw_configure.argtypes = [C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_uint64]
    lib.dg_hnsw_set_ef.argtypes = [C.c_void_p, C.c_int32]
    lib.dg_hnsw_get_info.argtypes = [C.c_void_p, C.POINTER(_HnswInfo)]
    lib.dg_search_hnsw.argtypes = lib.dg_search.argtypes
    lib.dg_search_hnsw_device.argtypes = lib.dg_search_device.argtypes
    lib.dg_hnsw_export_level.argtypes = [C.c_void_p, C.c_int32, _i32p, _u32p]
    lib.dg_hnsw_export_nodes.argtypes = [C.c_void_p, _i64p, _u8p, _i32p]
    lib.dg_hnsw_last_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64)]
    lib.dg_save_hnswlib.argtypes = [C.c_void_p, C.c_char_p]
    lib.dg_load_hnswlib.argtypes = [C.POINTER(C.c_void_p), C.c_char_p,
                                    C.c_int32, C.c_int32, C.c_int32]
    lib.dg_hnsw_max_elements.argtypes = [C.c_void_p, C.c_int64]
    lib.dg_hnsw_max_elements.restype = C.c_int64
    lib.dg_mirror_selftest_hnsw.restype = C.c_int
    return lib


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def last_error():
    buf = C.create_string_buffer(1024)
    lib().dg_last_error(buf, 1024)
    return buf.value.decode()


def _check(st, what):
    if st != 0:
        err = DgError(f"{what} failed (status {st}): {last_error()}")
        err.status = st  # dg_status code, for callers that dispatch on it
        raise err


def build_info():
    return lib().dg_build_info().decode()


def device_count():
    return lib().dg_device_count()


def ivfpq_max_m(device=0):
    """Largest IVF-PQ m whose scan tile fits the device's LDS."""
    l = lib()
    l.dg_ivfpq_max_m.argtypes = [C.c_int32]
    l.dg_ivfpq_max_m.restype = C.c_int32
    return l.dg_ivfpq_max_m(device)


def ivfpq_max_m_nbits(device=0, nbits=8):
    """The same limit for a code width (nbits 4 or 8; 0 for any other)."""
    l = lib()
    l.dg_ivfpq_max_m_nbits.argtypes = [C.c_int32, C.c_int32]
    l.dg_ivfpq_max_m_nbits.restype = C.c_int32
    return l.dg_ivfpq_max_m_nbits(device, nbits)


def make_filter(kind=0, negate=False, min_id=0, max_id=0, ids=None,
                bitmap=None, bitmap_base=0):
    f = _Filter()
    f.kind = kind
    f.negate = 1 if negate else 0
    f.min_id, f.max_id = min_id, max_id
    if ids is not None:
        ids = np.ascontiguousarray(ids, np.int64)
        f._ids_keepalive = ids  # not a ctypes field; python-side keepalive
        f.ids = ids.ctypes.data
        f.n_ids = len(ids)
    if bitmap is not None:
        bitmap = np.ascontiguousarray(bitmap, np.uint64)
        f._bm_keepalive = bitmap
        f.bitmap = bitmap.ctypes.data
        f.bitmap_base = bitmap_base
        f.bitmap_nbits = len(bitmap) * 64
    return f


class Index:
    def __init__(self, kind, metric, d, nlist=0, m=0, device=-1,
                 reserve=0, _handle=None, nbits=8, storage="f32"):
        """nbits: IVF-PQ bits per code, 4 or 8 (0 = the default 8).
        storage: "f32", or "f16" to keep the rows of an IVF_FLAT index as
        IEEE halves (dg_set_storage; half the memory and scan bytes, the
        distances are those to the rounded rows), or "sq8" for one byte per
        component (per-dimension 8-bit scalar quantisation; a quarter of the
        memory and scan bytes; train() or set_sq_ranges() gives the ranges,
        the distances are those to the decoded rows)."""
        code = _storage_code(storage)
        self.kind, self.metric, self.d = kind, metric, d
        self.nlist = nlist
        self.m = m
        self.nbits = nbits if nbits > 0 else 8
        if _handle is not None:
            self.h = _handle
            return
        desc = _Desc(kind=kind, metric=metric, d=d, nlist=nlist,
                     pq_m=m, pq_nbits=nbits, device=device, reserve=reserve)
        h = C.c_void_p()
        _check(lib().dg_index_create(C.byref(h), C.byref(desc)),
               "dg_index_create")
        self.h = h
        if code != STORAGE_F32:
            st = lib().dg_set_storage(self.h, code)
            if st != 0:
                msg = last_error()
                self.close()
                err = DgError(f"dg_set_storage failed (status {st}): {msg}")
                err.status = st
                raise err

    @property
    def storage(self):
        """"f32", "f16" or "sq8" (dg_get_storage)."""
        return {v: k for k, v in _STORAGE.items()}[
            lib().dg_get_storage(self.h)]

    def set_storage(self, storage):
        """Only while the index holds no rows (dg_set_storage)."""
        _check(lib().dg_set_storage(self.h, _storage_code(storage)),
               "dg_set_storage")

    def reconstruct(self, ids):
        """The stored rows of ids decoded to float32 [len(ids), d]; for
        COSINE the normalised rows.  Every id must be live."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        out = np.empty((len(ids), self.d), np.float32)
        _check(lib().dg_reconstruct(self.h, len(ids), ids, out),
               "dg_reconstruct")
        return out

    def set_sq_ranges(self, vmin, vdiff):
        """Per-dimension ranges of an empty SQ8 index (dg_set_sq_ranges)."""
        vmin = np.ascontiguousarray(vmin, np.float32).reshape(-1)
        vdiff = np.ascontiguousarray(vdiff, np.float32).reshape(-1)
        if len(vmin) != self.d or len(vdiff) != self.d:
            raise DgError(f"ranges must hold d = {self.d} values each")
        _check(lib().dg_set_sq_ranges(self.h, vmin, vdiff),
               "dg_set_sq_ranges")

    def get_sq_ranges(self):
        """(vmin, vdiff), float32 [d] each (dg_get_sq_ranges)."""
        vmin = np.empty(self.d, np.float32)
        vdiff = np.empty(self.d, np.float32)
        _check(lib().dg_get_sq_ranges(self.h, vmin, vdiff),
               "dg_get_sq_ranges")
        return vmin, vdiff

    def last_scan_sq8(self):
        """True if the last IVF-Flat search that ran its kernels scanned SQ8
        rows (dg_last_scan_sq8)."""
        return bool(lib().dg_last_scan_sq8(self.h))

    def last_scan_f16(self):
        """True if the last IVF-Flat search that ran its kernels scanned f16
        rows (dg_last_scan_f16)."""
        return bool(lib().dg_last_scan_f16(self.h))

    def close(self):
        if getattr(self, "h", None):
            # a shard view (ShardedIndex.shard) borrows its handle
            if not getattr(self, "_borrowed", False):
                lib().dg_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def is_binary(self):
        return self.kind in (BINARY_FLAT, BINARY_IVF_FLAT)

    def train(self, x):
        if self.is_binary:
            x = np.ascontiguousarray(x, np.uint8)
            _check(lib().dg_train_binary(self.h, x.shape[0], x),
                   "dg_train_binary")
            self.nlist = self.stats()["nlist"]  # n < nlist degrades to 1
            return
        x = np.ascontiguousarray(x, np.float32)
        _check(lib().dg_train(self.h, x.shape[0], x), "dg_train")

    def set_centroids(self, centroids):
        if self.is_binary:
            centroids = np.ascontiguousarray(centroids, np.uint8)
            _check(lib().dg_set_centroids_binary(
                self.h, centroids.shape[0], centroids),
                "dg_set_centroids_binary")
            self.nlist = centroids.shape[0]
            return
        centroids = np.ascontiguousarray(centroids, np.float32)
        self.nlist = centroids.shape[0]
        _check(lib().dg_set_centroids(self.h, centroids.shape[0], centroids),
               "dg_set_centroids")

    def get_centroids(self):
        if self.is_binary:
            out = np.empty((self.stats()["nlist"], self.d // 8), np.uint8)
            _check(lib().dg_get_centroids_binary(self.h, out),
                   "dg_get_centroids_binary")
            return out
        out = np.empty((self.nlist, self.d), np.float32)
        _check(lib().dg_get_centroids(self.h, out), "dg_get_centroids")
        return out

    def set_codebooks(self, codebooks):
        """codebooks: [m, 2**nbits, d//m] float32."""
        cb = np.ascontiguousarray(codebooks, np.float32)
        self.m = cb.shape[0]
        l = lib()
        l.dg_set_codebooks.argtypes = [C.c_void_p, C.c_int32, C.c_int32,
                                       _f32p]
        if cb.ndim != 3 or cb.shape[1] != 1 << self.nbits:
            raise DgError(f"codebooks must be [m, {1 << self.nbits}, d//m] "
                          f"at nbits={self.nbits}, got {cb.shape}")
        _check(l.dg_set_codebooks(self.h, cb.shape[0], self.nbits,
                                  cb.reshape(-1)),
               "dg_set_codebooks")

    def get_codebooks(self):
        dsub = self.d // self.m
        out = np.empty((self.m, 1 << self.nbits, dsub), np.float32)
        l = lib()
        l.dg_get_codebooks.argtypes = [C.c_void_p, _f32p]
        _check(l.dg_get_codebooks(self.h, out.reshape(-1)),
               "dg_get_codebooks")
        return out

    def add(self, ids, x):
        ids = np.ascontiguousarray(ids, np.int64)
        if self.is_binary:
            x = np.ascontiguousarray(x, np.uint8)
            _check(lib().dg_add_binary(self.h, x.shape[0], ids, x),
                   "dg_add_binary")
            return
        x = np.ascontiguousarray(x, np.float32)
        _check(lib().dg_add(self.h, x.shape[0], ids, x), "dg_add")

    def add_device(self, ids, x_ptr, n):
        """Add n vectors from a device pointer (torch .data_ptr())."""
        ids = np.ascontiguousarray(ids, np.int64)
        l = lib()
        l.dg_add_device.argtypes = [C.c_void_p, C.c_int64, _i64p, C.c_void_p]
        _check(l.dg_add_device(self.h, n, ids, C.c_void_p(x_ptr)),
               "dg_add_device")

    def export_assign(self):
        l = lib()
        l.dg_export_assign.argtypes = [
            C.c_void_p, np.ctypeslib.ndpointer(np.int32,
                                               flags="C_CONTIGUOUS")]
        st = self.stats()
        # arrival order, tombstoned rows included (dg_export_assign)
        out = np.empty(st["ntotal"] + st["deleted_count"], np.int32)
        _check(l.dg_export_assign(self.h, out), "dg_export_assign")
        return out

    def upsert(self, ids, x):
        ids = np.ascontiguousarray(ids, np.int64)
        if self.is_binary:
            x = np.ascontiguousarray(x, np.uint8)
            _check(lib().dg_upsert_binary(self.h, x.shape[0], ids, x),
                   "dg_upsert_binary")
            return
        x = np.ascontiguousarray(x, np.float32)
        _check(lib().dg_upsert(self.h, x.shape[0], ids, x), "dg_upsert")

    def remove(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        _check(lib().dg_remove(self.h, len(ids), ids), "dg_remove")

    def search(self, queries, k, nprobe=0, filt=None):
        """Binary indexes take np.uint8 [nq, d // 8] queries and return the
        integer Hamming distance as float32."""
        q = np.ascontiguousarray(
            queries, np.uint8 if self.is_binary else np.float32)
        nq = q.shape[0]
        dist = np.empty((nq, k), np.float32)
        ids = np.empty((nq, k), np.int64)
        fp = C.byref(filt) if filt is not None else None
        if self.is_binary:
            _check(lib().dg_search_binary(self.h, nq, q, k, nprobe, fp, dist,
                                          ids), "dg_search_binary")
            return dist, ids
        _check(lib().dg_search(self.h, nq, q, k, nprobe, fp, dist, ids),
               "dg_search")
        return dist, ids

    def enable_batching(self, max_batch=0, max_wait_us=0):
        """Coalesce concurrent search_batched calls of this index into device
        batches (dg_batching_enable).  max_batch 0 = 64 queries per batch;
        max_wait_us 0 = a batch never waits for company once the device is
        free.  Enabling again drains and restarts the statistics."""
        opts = _BatchOpts(max_batch=max_batch, max_wait_us=max_wait_us)
        _check(lib().dg_batching_enable(self.h, C.byref(opts)),
               "dg_batching_enable")

    def disable_batching(self):
        """Wait for the open batches; later search_batched calls are plain
        searches."""
        _check(lib().dg_batching_disable(self.h), "dg_batching_disable")

    def batching_stats(self):
        s = _BatchStats()
        _check(lib().dg_batching_stats(self.h, C.byref(s)),
               "dg_batching_stats")
        return {f[0]: getattr(s, f[0]) for f in _BatchStats._fields_}

    def search_batched(self, queries, k, nprobe=0, filt=None):
        """search() for callers on many threads with few queries each: with
        batching enabled, calls that wait together run as one device batch
        and each returns its own rows.  ctypes releases the GIL for the
        call, so Python threads do block and merge here.  Without
        enable_batching() it is search()."""
        q = np.ascontiguousarray(
            queries, np.uint8 if self.is_binary else np.float32)
        nq = q.shape[0]
        dist = np.empty((nq, k), np.float32)
        ids = np.empty((nq, k), np.int64)
        fp = C.byref(filt) if filt is not None else None
        if self.is_binary:
            _check(lib().dg_search_binary_batched(
                self.h, nq, q, k, nprobe, fp, dist, ids),
                "dg_search_binary_batched")
            return dist, ids
        _check(lib().dg_search_batched(self.h, nq, q, k, nprobe, fp, dist,
                                       ids), "dg_search_batched")
        return dist, ids

    def search_device(self, q_ptr, nq, k, nprobe, dist_ptr, ids_ptr,
                      filt=None):
        """Device-pointer hot path (pointers = torch .data_ptr())."""
        fp = C.byref(filt) if filt is not None else None
        if self.is_binary:
            _check(lib().dg_search_binary_device(
                self.h, nq, C.c_void_p(q_ptr), k, nprobe, fp,
                C.c_void_p(dist_ptr), C.c_void_p(ids_ptr)),
                "dg_search_binary_device")
            return
        _check(lib().dg_search_device(self.h, nq, C.c_void_p(q_ptr), k,
                                      nprobe, fp, C.c_void_p(dist_ptr),
                                      C.c_void_p(ids_ptr)),
               "dg_search_device")

    def range_search(self, queries, radius, filt=None):
        """Radius search (faiss convention: L2 dist < r; IP score > r).
        Returns (lims[nq+1], dists, ids) with per-query best-first order."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        lims = np.zeros(nq + 1, np.int64)
        out_ids = C.POINTER(C.c_int64)()
        out_dists = C.POINTER(C.c_float)()
        l = lib()
        l.dg_range_search.argtypes = [
            C.c_void_p, C.c_int64, _f32p, C.c_float, C.POINTER(_Filter),
            _i64p, C.POINTER(C.POINTER(C.c_int64)),
            C.POINTER(C.POINTER(C.c_float)),
        ]
        l.dg_free.argtypes = [C.c_void_p]
        fp = C.byref(filt) if filt is not None else None
        _check(l.dg_range_search(self.h, nq, q, radius, fp, lims,
                                 C.byref(out_ids), C.byref(out_dists)),
               "dg_range_search")
        total = int(lims[-1])
        dists = np.ctypeslib.as_array(out_dists, (max(total, 1),))[
            :total].copy()
        ids = np.ctypeslib.as_array(out_ids, (max(total, 1),))[:total].copy()
        l.dg_free(C.cast(out_ids, C.c_void_p))
        l.dg_free(C.cast(out_dists, C.c_void_p))
        return lims, dists, ids

    def range_search_binary(self, queries_u8, radius, nprobe=0, filt=None):
        """Binary radius search: rows with hamming(query, row) < radius
        (an integer).  Returns (lims[nq+1], dists, ids), per query ascending
        by (distance, id); dists are the integer distances as float32."""
        q = np.ascontiguousarray(queries_u8, np.uint8)
        nq = q.shape[0]
        lims = np.zeros(nq + 1, np.int64)
        out_ids = C.POINTER(C.c_int64)()
        out_dists = C.POINTER(C.c_float)()
        l = lib()
        fp = C.byref(filt) if filt is not None else None
        st = l.dg_range_search_binary(self.h, nq, q, int(radius), nprobe, fp,
                                      lims, C.byref(out_ids),
                                      C.byref(out_dists))
        try:
            _check(st, "dg_range_search_binary")
            total = int(lims[-1])
            if total:
                dists = np.ctypeslib.as_array(out_dists, (total,)).copy()
                ids = np.ctypeslib.as_array(out_ids, (total,)).copy()
            else:
                dists = np.empty(0, np.float32)
                ids = np.empty(0, np.int64)
        finally:
            l.dg_free(C.cast(out_ids, C.c_void_p))
            l.dg_free(C.cast(out_dists, C.c_void_p))
        return lims, dists, ids

    def sync(self):
        _check(lib().dg_sync(self.h), "dg_sync")

    # ---- HNSW (kind HNSW) ----
    def hnsw_configure(self, nlinks=32, ef_construction=200, seed=100):
        """Graph parameters, only while the index is empty
        (dg_hnsw_configure): nlinks 2..128, ef_construction 1..4096."""
        _check(lib().dg_hnsw_configure(self.h, nlinks, ef_construction, seed),
               "dg_hnsw_configure")

    def set_ef(self, ef_search):
        """The stored ef_search (1..1024) that search() and ef_search = 0
        use (dg_hnsw_set_ef)."""
        _check(lib().dg_hnsw_set_ef(self.h, ef_search), "dg_hnsw_set_ef")

    def hnsw_info(self):
        s = _HnswInfo()
        _check(lib().dg_hnsw_get_info(self.h, C.byref(s)),
               "dg_hnsw_get_info")
        return {f[0]: getattr(s, f[0]) for f in _HnswInfo._fields_}

    def search_hnsw(self, queries, k, ef_search=0, filt=None):
        """Graph search with a beam of max(ef_search, k); ef_search 0 = the
        stored value.  Returns (dist, ids) like search()."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        dist = np.empty((nq, max(k, 0)), np.float32)
        ids = np.empty((nq, max(k, 0)), np.int64)
        fp = C.byref(filt) if filt is not None else None
        _check(lib().dg_search_hnsw(self.h, nq, q, k, ef_search, fp, dist,
                                    ids), "dg_search_hnsw")
        return dist, ids

    def search_hnsw_device(self, q_ptr, nq, k, ef_search, dist_ptr, ids_ptr,
                           filt=None):
        """Device-pointer form, no synchronisation (sync() waits)."""
        fp = C.byref(filt) if filt is not None else None
        _check(lib().dg_search_hnsw_device(
            self.h, nq, C.c_void_p(q_ptr), k, ef_search, fp,
            C.c_void_p(dist_ptr), C.c_void_p(ids_ptr)),
            "dg_search_hnsw_device")

    def hnsw_export(self):
        """The graph as the DEVICE holds it: dict(ids, deleted, levels,
        counts, links, entry_point, max_level, nlinks); counts[l] is [n]
        int32 (-1: the node has no level l), links[l] is [n, cap(l)] uint32,
        for l = 0 .. max_level (dg_hnsw_export_nodes / _level)."""
        info = self.hnsw_info()
        n = info["n_nodes"]
        ids = np.zeros(n, np.int64)
        deleted = np.zeros(n, np.uint8)
        levels = np.zeros(n, np.int32)
        _check(lib().dg_hnsw_export_nodes(self.h, ids, deleted, levels),
               "dg_hnsw_export_nodes")
        counts, links = [], []
        for level in range(max(info["max_level"], 0) + 1):
            cap = info["max_m0"] if level == 0 else info["nlinks"]
            c = np.zeros(n, np.int32)
            lk = np.zeros((n, cap), np.uint32)
            _check(lib().dg_hnsw_export_level(self.h, level, c, lk),
                   "dg_hnsw_export_level")
            counts.append(c)
            links.append(lk)
        return dict(ids=ids, deleted=deleted, levels=levels, counts=counts,
                    links=links, entry_point=info["entry_point"],
                    max_level=info["max_level"], nlinks=info["nlinks"])

    def hnsw_last_counters(self):
        """(expansions, dist_evals) summed over the last search's batch."""
        a, b = C.c_int64(), C.c_int64()
        _check(lib().dg_hnsw_last_counters(self.h, C.byref(a), C.byref(b)),
               "dg_hnsw_last_counters")
        return a.value, b.value

    def save_hnswlib(self, path):
        """hnswlib's saveIndex container (what the reference's HNSW
        snapshots are)."""
        _check(lib().dg_save_hnswlib(self.h, path.encode()),
               "dg_save_hnswlib")

    @classmethod
    def load_hnswlib(cls, path, metric, d, device=-1):
        """The file carries neither metric nor d: pass both."""
        h = C.c_void_p()
        _check(lib().dg_load_hnswlib(C.byref(h), path.encode(), metric, d,
                                     device), "dg_load_hnswlib")
        return cls._from_handle(h)

    def set_list_mask(self, mask):
        if mask is None:
            _check(lib().dg_set_list_mask(self.h, None), "dg_set_list_mask")
        else:
            mask = np.ascontiguousarray(mask, np.uint8)
            _check(lib().dg_set_list_mask(self.h, mask.ctypes.data),
                   "dg_set_list_mask")

    def save(self, path):
        _check(lib().dg_save(self.h, path.encode()), "dg_save")

    @classmethod
    def load(cls, path, device=-1):
        h = C.c_void_p()
        _check(lib().dg_load(C.byref(h), path.encode(), device), "dg_load")
        return cls._from_handle(h)

    def save_faiss(self, path):
        """Write a faiss-1.7.x-compatible container (the snapshot format the
        reference ships between nodes, vector_index_snapshot_manager.cc)."""
        l = lib()
        l.dg_save_faiss.argtypes = [C.c_void_p, C.c_char_p]
        _check(l.dg_save_faiss(self.h, path.encode()), "dg_save_faiss")

    @classmethod
    def load_faiss(cls, path, metric=-1, device=-1):
        """Load a faiss container (IxM2{IndexFlat} / IwFl / IwPQ).  metric
        = COSINE reinterprets an IP-metric file as a cosine index (the
        reference stores cosine as IP over normalized vectors)."""
        l = lib()
        l.dg_load_faiss.argtypes = [C.POINTER(C.c_void_p), C.c_char_p,
                                    C.c_int32, C.c_int32]
        h = C.c_void_p()
        _check(l.dg_load_faiss(C.byref(h), path.encode(), metric, device),
               "dg_load_faiss")
        return cls._from_handle(h)

    def save_faiss_binary(self, path):
        """Write the binary index as a faiss write_index_binary container
        (IndexBinaryIDMap2{IndexBinaryFlat} or IndexBinaryIVF)."""
        _check(lib().dg_save_faiss_binary(self.h, path.encode()),
               "dg_save_faiss_binary")

    @classmethod
    def load_faiss_binary(cls, path, device=-1):
        """Load a binary faiss container (IBM2/IBMp{IBxF} or IBwF)."""
        h = C.c_void_p()
        _check(lib().dg_load_faiss_binary(C.byref(h), path.encode(), device),
               "dg_load_faiss_binary")
        return cls._from_handle(h)

    @classmethod
    def _from_handle(cls, h):
        idx = cls.__new__(cls)
        idx.h = h
        st = idx.stats()
        idx.kind, idx.metric = st["kind"], st["metric"]
        idx.d, idx.nlist = st["d"], st["nlist"]
        idx.m, idx.nbits = 0, 8
        if idx.kind == IVF_PQ:  # restore the PQ geometry from the handle
            m, nbits = C.c_int32(), C.c_int32()
            l = lib()
            l.dg_pq_params.argtypes = [C.c_void_p, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32)]
            _check(l.dg_pq_params(h, C.byref(m), C.byref(nbits)),
                   "dg_pq_params")
            idx.m, idx.nbits = m.value, nbits.value
        return idx

    def last_scan_fused(self):
        """True if the last IVF search that ran its kernels kept the
        per-wave top-k inside the scan (see dg_last_scan_fused)."""
        l = lib()
        l.dg_last_scan_fused.argtypes = [C.c_void_p]
        l.dg_last_scan_fused.restype = C.c_int
        return bool(l.dg_last_scan_fused(self.h))

    def last_scan_mfma(self):
        """True if that fused scan ran the f32-MFMA kernel, False for the
        VALU kernel (DG_SCAN_MFMA=0) or an unfused search."""
        l = lib()
        l.dg_last_scan_mfma.argtypes = [C.c_void_p]
        l.dg_last_scan_mfma.restype = C.c_int
        return bool(l.dg_last_scan_mfma(self.h))

    def last_scan_pair(self):
        """True if the last search also launched the pair scan (two query
        tiles per pass on lists probed by 17+ queries); False with
        DG_SCAN_PAIR=0, nq <= 16, d > 2304 or without the MFMA scan."""
        l = lib()
        l.dg_last_scan_pair.argtypes = [C.c_void_p]
        l.dg_last_scan_pair.restype = C.c_int
        return bool(l.dg_last_scan_pair(self.h))

    def last_coarse_wave(self):
        """True if the last IVF search that ran its kernels selected its
        probes with k_coarse_select; False with DG_COARSE_WAVE=0, nprobe
        above the kernel's cap or nprobe >= nlist (dg_last_coarse_wave)."""
        l = lib()
        l.dg_last_coarse_wave.argtypes = [C.c_void_p]
        l.dg_last_coarse_wave.restype = C.c_int
        return bool(l.dg_last_coarse_wave(self.h))

    def last_probes(self):
        """The last IVF search's probes, int32 in selection order, -1 for a
        masked list, as one flat array of nq * nprobe entries
        (dg_last_probes; a debugging accessor)."""
        l = lib()
        l.dg_last_probes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        l.dg_last_probes.restype = C.c_int64
        out = np.empty(max(l.dg_last_probes(self.h, None, 0), 0), np.int32)
        if l.dg_last_probes(self.h, out.ctypes.data, out.size) != out.size:
            raise DgError("dg_last_probes: " + last_error())
        return out

    def stats(self):
        s = _Stats()
        _check(lib().dg_stats(self.h, C.byref(s)), "dg_stats")
        return {f[0]: getattr(s, f[0]) for f in _Stats._fields_
                if not f[0].startswith("_")}


def merge_topk(dists, ids, k, metric=L2):
    """Merge per-shard top-k results (the RCCL all-gather consumer).

    dists/ids: arrays [n_shards, nq, k] in faiss convention (L2 raw asc
    best; IP raw score desc best).  Returns merged [nq, k].
    Mirrors the reference's client-side region-scatter merge.
    """
    dists = np.asarray(dists)
    ids = np.asarray(ids)
    S, nq, kk = dists.shape
    cat_d = dists.transpose(1, 0, 2).reshape(nq, S * kk)
    cat_i = ids.transpose(1, 0, 2).reshape(nq, S * kk)
    key = cat_d if metric == L2 else -cat_d
    key = np.where(cat_i < 0, np.inf, key)
    order = np.lexsort((cat_i, key), axis=1)[:, :k]
    return (np.take_along_axis(cat_d, order, 1),
            np.take_along_axis(cat_i, order, 1))


def merge_topk_device(dists, ids, k, metric=L2, device=-1):
    """merge_topk on the GPU (dg_merge_topk): dists / ids [n_lists, nq,
    k_in], each list best-first with -1 / 0.0 pads behind the real rows.
    Returns the k best per query under the library's merge order (is_pad,
    key, list, position): ties between lists go to the smaller list, not to
    the smaller id as in the numpy merge_topk.  Real distances keep their
    bits; pads come out as -1 / 0.0."""
    d = np.ascontiguousarray(dists, np.float32)
    i = np.ascontiguousarray(ids, np.int64)
    if d.ndim != 3 or d.shape != i.shape:
        raise DgError(f"dists / ids must be [n_lists, nq, k_in], got "
                      f"{d.shape} and {i.shape}")
    n_lists, nq, k_in = d.shape
    od = np.empty((nq, k), np.float32)
    oi = np.empty((nq, k), np.int64)
    _check(lib().dg_merge_topk(n_lists, nq, k_in, k, metric, d, i, od, oi,
                               device), "dg_merge_topk")
    return od, oi


def shard_of(ids, n_shards):
    """The shard of each id in a ShardedIndex of n_shards shards: the
    splitmix64 finaliser of the id, modulo n_shards (dg_shard_of)."""
    with np.errstate(over="ignore"):
        z = np.asarray(ids, np.int64).astype(np.uint64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z % np.uint64(n_shards)).astype(np.int32)


class ShardedIndex:
    """One index over several GPUs of this process (dg_sharded_*): a shard
    per entry of `devices` (ordinals may repeat), rows routed by id, search
    fanned out and merged on the first shard's device.  Float kinds only;
    no save / load, no search batching, no list mask."""

    def __init__(self, kind, metric, d, devices, nlist=0, m=0, nbits=8,
                 reserve=0, storage="f32"):
        code = _storage_code(storage)
        self.kind, self.metric, self.d = kind, metric, d
        self.nlist, self.m = nlist, m
        self.nbits = nbits if nbits > 0 else 8
        devs = np.ascontiguousarray(devices, np.int32).reshape(-1)
        self.n_shards = len(devs)
        desc = _Desc(kind=kind, metric=metric, d=d, nlist=nlist, pq_m=m,
                     pq_nbits=nbits, device=-1, reserve=reserve)
        h = C.c_void_p()
        # an empty device list still reaches the library's n_shards check
        _check(lib().dg_sharded_create(
            C.byref(h), C.byref(desc), self.n_shards,
            devs if len(devs) else np.zeros(1, np.int32)),
            "dg_sharded_create")
        self.h = h
        if code != STORAGE_F32:
            st = lib().dg_sharded_set_storage(self.h, code)
            if st != 0:
                msg = last_error()
                self.close()
                err = DgError(
                    f"dg_sharded_set_storage failed (status {st}): {msg}")
                err.status = st
                raise err

    def close(self):
        if getattr(self, "h", None):
            lib().dg_sharded_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def train(self, x):
        x = np.ascontiguousarray(x, np.float32)
        _check(lib().dg_sharded_train(self.h, x.shape[0], x),
               "dg_sharded_train")
        if self.kind != FLAT:
            self.nlist = self.stats()["nlist"]  # n < nlist degrades to 1

    def set_centroids(self, centroids):
        c = np.ascontiguousarray(centroids, np.float32)
        _check(lib().dg_sharded_set_centroids(self.h, c.shape[0], c),
               "dg_sharded_set_centroids")
        self.nlist = c.shape[0]

    def get_centroids(self):
        out = np.empty((self.nlist, self.d), np.float32)
        _check(lib().dg_sharded_get_centroids(self.h, out),
               "dg_sharded_get_centroids")
        return out

    def set_sq_ranges(self, vmin, vdiff):
        """The SQ8 ranges of every (empty) shard."""
        vmin = np.ascontiguousarray(vmin, np.float32).reshape(-1)
        vdiff = np.ascontiguousarray(vdiff, np.float32).reshape(-1)
        if len(vmin) != self.d or len(vdiff) != self.d:
            raise DgError(f"ranges must hold d = {self.d} values each")
        _check(lib().dg_sharded_set_sq_ranges(self.h, vmin, vdiff),
               "dg_sharded_set_sq_ranges")

    def get_sq_ranges(self):
        """(vmin, vdiff) of shard 0; every shard holds the same."""
        vmin = np.empty(self.d, np.float32)
        vdiff = np.empty(self.d, np.float32)
        _check(lib().dg_sharded_get_sq_ranges(self.h, vmin, vdiff),
               "dg_sharded_get_sq_ranges")
        return vmin, vdiff

    def set_codebooks(self, codebooks):
        """codebooks: [m, 2**nbits, d//m] float32."""
        cb = np.ascontiguousarray(codebooks, np.float32)
        if cb.ndim != 3 or cb.shape[1] != 1 << self.nbits:
            raise DgError(f"codebooks must be [m, {1 << self.nbits}, d//m] "
                          f"at nbits={self.nbits}, got {cb.shape}")
        self.m = cb.shape[0]
        _check(lib().dg_sharded_set_codebooks(self.h, cb.shape[0], self.nbits,
                                              cb.reshape(-1)),
               "dg_sharded_set_codebooks")

    def get_codebooks(self):
        out = np.empty((self.m, 1 << self.nbits, self.d // self.m),
                       np.float32)
        _check(lib().dg_sharded_get_codebooks(self.h, out.reshape(-1)),
               "dg_sharded_get_codebooks")
        return out

    def add(self, ids, x):
        ids = np.ascontiguousarray(ids, np.int64)
        x = np.ascontiguousarray(x, np.float32)
        _check(lib().dg_sharded_add(self.h, x.shape[0], ids, x),
               "dg_sharded_add")

    def upsert(self, ids, x):
        ids = np.ascontiguousarray(ids, np.int64)
        x = np.ascontiguousarray(x, np.float32)
        _check(lib().dg_sharded_upsert(self.h, x.shape[0], ids, x),
               "dg_sharded_upsert")

    def remove(self, ids):
        ids = np.ascontiguousarray(ids, np.int64)
        _check(lib().dg_sharded_remove(self.h, len(ids), ids),
               "dg_sharded_remove")

    def search(self, queries, k, nprobe=0, filt=None):
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        dist = np.empty((nq, max(k, 0)), np.float32)
        ids = np.empty((nq, max(k, 0)), np.int64)
        fp = C.byref(filt) if filt is not None else None
        _check(lib().dg_sharded_search(self.h, nq, q, k, nprobe, fp, dist,
                                       ids), "dg_sharded_search")
        return dist, ids

    def search_device(self, q_ptr, nq, k, nprobe, dist_ptr, ids_ptr,
                      filt=None):
        """Device-pointer form: pointers on the first shard's device; the
        merge is enqueued on the handle's merge stream (sync() waits)."""
        fp = C.byref(filt) if filt is not None else None
        _check(lib().dg_sharded_search_device(
            self.h, nq, C.c_void_p(q_ptr), k, nprobe, fp,
            C.c_void_p(dist_ptr), C.c_void_p(ids_ptr)),
            "dg_sharded_search_device")

    def sync(self):
        _check(lib().dg_sharded_sync(self.h), "dg_sharded_sync")

    def range_search(self, queries, radius, filt=None):
        """Returns (lims[nq+1], dists, ids), per query best-first with ties
        toward the smaller id, like Index.range_search."""
        q = np.ascontiguousarray(queries, np.float32)
        nq = q.shape[0]
        lims = np.zeros(nq + 1, np.int64)
        out_ids = C.POINTER(C.c_int64)()
        out_dists = C.POINTER(C.c_float)()
        l = lib()
        fp = C.byref(filt) if filt is not None else None
        st = l.dg_sharded_range_search(self.h, nq, q, radius, fp, lims,
                                       C.byref(out_ids), C.byref(out_dists))
        try:
            _check(st, "dg_sharded_range_search")
            total = int(lims[-1])
            if total:
                dists = np.ctypeslib.as_array(out_dists, (total,)).copy()
                ids = np.ctypeslib.as_array(out_ids, (total,)).copy()
            else:
                dists = np.empty(0, np.float32)
                ids = np.empty(0, np.int64)
        finally:
            l.dg_free(C.cast(out_ids, C.c_void_p))
            l.dg_free(C.cast(out_dists, C.c_void_p))
        return lims, dists, ids

    def stats(self):
        s = _Stats()
        _check(lib().dg_sharded_stats(self.h, C.byref(s)), "dg_sharded_stats")
        return {f[0]: getattr(s, f[0]) for f in _Stats._fields_
                if not f[0].startswith("_")}

    def shard(self, i):
        """Shard i as an Index that borrows the handle: for stats(),
        get_centroids(), export_assign() and read-only searches.  It stays
        valid until this ShardedIndex is closed."""
        h = lib().dg_sharded_shard(self.h, i)
        if not h:
            raise DgError(f"shard {i} out of range (n_shards "
                          f"{self.n_shards})")
        idx = Index._from_handle(C.c_void_p(h))
        idx._borrowed = True
        return idx
