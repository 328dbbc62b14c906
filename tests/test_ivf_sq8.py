"""IVF-Flat with SQ8 row storage (DG_STORAGE_SQ8) on the GPU (marked gpu).

Codec: the codes recovered from reconstruct equal the float64 codec's away
from code boundaries, a decoded component is within 4u (|vmin| + vdiff) of
the float64 decode, out-of-range components saturate, a flat dimension
(vdiff = 0) decodes to vmin; dg_train yields the min and max - min of its
rows.  Scan: k_ivf_scan_sq8 in its fused and its store-all form, every query
of every search held to rules A-D (or the range rules) of flat_reference over
the verified assignment, against the float64 reference over the f32 queries
and the rows the index returns from reconstruct, within the derived bound b8
(ivf_sq8_reference).  The searches are the drivers of ivf_reference, which
test_ivf_sq8_cpu.py runs dry.  Contract: the refusals of set_storage and
set_sq_ranges, the trained state, the finite check of add and upsert, save /
load, search_batched, the sharded index and the mirror.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO, os.path.join(REPO, "dingo-store_amd")]

pytestmark = pytest.mark.gpu

import dingostore as dg  # noqa: E402
import flat_reference as fr  # noqa: E402
import ivf_reference as ir  # noqa: E402
import ivf_sq8_reference as h8  # noqa: E402
from flat_reference import COSINE, IP, L2, U  # noqa: E402

MNAME = {L2: "L2", IP: "IP", COSINE: "COSINE"}
DG_EINVAL, DG_ENOT_TRAINED, DG_ENOT_SUPPORT, DG_ENOT_FOUND = 1, 2, 3, 9


@pytest.fixture(scope="module", autouse=True)
def _report_slack():
    yield
    print("\nIVF-Flat SQ8: largest |dist - ref| / b8 per metric:",
          {MNAME[m]: round(v, 4) for m, v in h8.MAX_RATIO.items()})


@pytest.fixture(autouse=True)
def _default_scan_path(monkeypatch):
    monkeypatch.delenv("DG_SCAN_FUSED", raising=False)
    monkeypatch.delenv("DG_SCAN_F16_PY", raising=False)


def _status(fn, *a, **kw):
    with pytest.raises(dg.DgError) as e:
        fn(*a, **kw)
    return e.value.status


def make_dg_filter(spec):
    if spec is None:
        return None
    if spec["kind"] == 1:
        return dg.make_filter(kind=1, negate=spec["negate"],
                              min_id=spec["min_id"], max_id=spec["max_id"])
    if spec["kind"] == 2:
        return dg.make_filter(kind=2, negate=spec["negate"], ids=spec["ids"])
    f = dg.make_filter(kind=3, negate=spec["negate"], bitmap=spec["bitmap"],
                       bitmap_base=spec["bitmap_base"])
    f.bitmap_nbits = spec["bitmap_nbits"]  # not a multiple of 64
    return f


def _ranges(c):
    rows = h8.normalize_f32(c.x) if c.metric == COSINE else c.x
    return h8.ranges_of(rows)


def _index(c, storage="sq8"):
    idx = dg.Index(dg.IVF_FLAT, c.metric, c.d, nlist=c.nlist,
                   storage=storage)
    idx.set_centroids(c.cents)
    if storage == "sq8":
        idx.set_sq_ranges(*_ranges(c))
    idx.add(c.ids, c.x)
    return idx


class GpuOps8:
    """The driver operations of ivf_reference on an SQ8 index; the case the
    drivers see carries (ref, b8) over the rows reconstruct returns."""

    def __init__(self, c):
        self.idx = _index(c)
        assert self.idx.storage == "sq8"
        self.c = h8.sq8_case(c, self.idx.reconstruct(c.ids))
        vmin, vdiff = self.idx.get_sq_ranges()
        assert np.array_equal(vmin, self.c.vmin)
        assert np.array_equal(vdiff, self.c.vdiff)
        self.searches = 0

    def verified_assign(self):
        c = self.c
        assign = self.idx.export_assign()
        # rows are assigned from their f32 values, not from the codes
        ir.verify_assign(c.metric, c.x, c.cents, assign,
                         (MNAME[c.metric], c.d))
        assert np.array_equal(np.bincount(assign, minlength=c.nlist), c.lens)
        return assign

    def search(self, where, q, k, nprobe, spec, ref, b, ids, elig, fused):
        gd, gi = self.idx.search(q, k, nprobe=nprobe,
                                 filt=make_dg_filter(spec))
        assert self.idx.last_scan_fused() == fused, where
        assert self.idx.last_scan_sq8() and not self.idx.last_scan_pair()
        assert not self.idx.last_scan_f16()
        h8.check_topk(self.c.metric, gd, gi, ref, b, ids, elig, where)
        self.searches += 1

    def range_search(self, where, q, radius, ref, b, ids, elig):
        lims, rd, ri = self.idx.range_search(q, radius)
        assert not self.idx.last_scan_fused() and self.idx.last_scan_sq8()
        h8.check_range(self.c.metric, radius, lims, rd, ri, ref, b, ids,
                       elig, where)
        self.searches += 1

    def remove(self, ids):
        self.idx.remove(ids)

    def upsert(self, ids, vectors):
        self.idx.upsert(ids, vectors)

    def replayed(self, where, expected):
        assert (self.idx.stats()["last_nq"] == 0) == expected, where

    def close(self):
        self.idx.close()


def _run(c, driver, *args, **kw):
    ops = GpuOps8(c)
    try:
        if kw.get("reconstruct"):
            driver(ops.c, ops.verified_assign(), ops, *args,
                   reconstruct=ops.idx.reconstruct)
        else:
            driver(ops.c, ops.verified_assign(), ops, *args)
        assert ops.searches > 0
    finally:
        ops.close()


# --------------------------------------------------------------------------
# codec on the device
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP], ids=lambda m: MNAME[m])
@pytest.mark.parametrize("d", [5, 32, 100])
def test_codec_on_the_device(d, metric):
    c = ir.case_a(d, metric)
    lo, w = h8.ranges_of(c.x)
    # ranges injected, widened by 1/64 of vdiff on each side
    vmin = (lo - w / np.float32(64)).astype(np.float32)
    vdiff = (w * np.float32(1 + 2 / 64)).astype(np.float32)
    flat = d - 1  # a flat dimension: every component decodes to vmin
    vdiff[flat] = 0.0
    x = c.x.copy()
    # row 0 saturates low, row 1 high, in every dimension
    x[0] = vmin - np.float32(3) * np.maximum(vdiff, 1)
    x[1] = vmin + np.float32(4) * np.maximum(vdiff, 1)
    idx = dg.Index(dg.IVF_FLAT, metric, d, nlist=c.nlist, storage="sq8")
    try:
        idx.set_centroids(c.cents)
        idx.set_sq_ranges(vmin, vdiff)
        g0, g1 = idx.get_sq_ranges()
        assert np.array_equal(g0, vmin) and np.array_equal(g1, vdiff)
        idx.add(c.ids, x)
        r = idx.reconstruct(c.ids)
        assert r.shape == x.shape and r.dtype == np.float32
        # repeated ids, any order
        pick = c.ids[[7, 3, 7, c.n - 1]]
        assert np.array_equal(idx.reconstruct(pick), r[[7, 3, 7, c.n - 1]])
    finally:
        idx.close()
    lo64, w64 = vmin.astype(np.float64), vdiff.astype(np.float64)
    live = w64 > 0
    step = np.where(live, w64 / 255.0, 1.0)
    got = np.where(live[None, :],
                   np.round((r.astype(np.float64) - lo64) / step - 0.5), 0.0)
    assert ((got >= 0) & (got <= 255)).all()
    # the flat dimension: code 0 decodes to vmin exactly
    assert (r[:, flat] == vmin[flat]).all()
    # saturation
    assert (got[0] == 0).all() and (got[1, live] == 255).all()
    # the f64 codec's codes, except within 1e-3 of a code boundary
    t = h8.encode_t(x, vmin, vdiff)
    want = np.floor(t)
    near = np.abs(t - np.round(t)) <= 1e-3
    body = np.ones(x.shape, bool)
    body[:2] = False          # the saturated rows are checked above
    body[:, ~live] = False
    left_out = (near & body).sum() / body.sum()
    print("components left out:", left_out)
    assert left_out <= 0.01
    use = body & ~near
    assert np.array_equal(got[use], want[use])
    # every decoded component is the f32 decode of its code
    dec = h8.decode(got, vmin, vdiff)
    assert (np.abs(r.astype(np.float64) - dec) <=
            4 * U * (np.abs(lo64) + w64)[None, :]).all()


@pytest.mark.parametrize("metric", [L2, IP, COSINE], ids=lambda m: MNAME[m])
def test_train_yields_min_and_max_of_the_rows(metric):
    c = ir.case_c(metric)
    idx = dg.Index(dg.IVF_FLAT, metric, c.d, nlist=c.nlist, storage="sq8")
    try:
        assert not idx.stats()["is_trained"]
        assert _status(idx.get_sq_ranges) == DG_ENOT_TRAINED
        idx.set_centroids(c.cents)
        # centroids alone do not make an SQ8 index trained
        assert not idx.stats()["is_trained"]
        assert _status(idx.add, c.ids[:4], c.x[:4]) == DG_ENOT_TRAINED
        assert _status(idx.upsert, c.ids[:4], c.x[:4]) == DG_ENOT_TRAINED
        gd, gi = idx.search(c.q[:3], 5, nprobe=3)  # blank, OK
        assert (gi == -1).all()
        idx.train(c.x)  # centroids are present: trains the ranges only
        assert idx.stats()["is_trained"]
        assert np.array_equal(idx.get_centroids().view(np.uint32),
                              c.cents.view(np.uint32))
        vmin, vdiff = idx.get_sq_ranges()
        if metric != COSINE:
            lo = c.x.min(0)
            assert np.array_equal(vmin.view(np.uint32), lo.view(np.uint32))
            assert np.array_equal(vdiff.view(np.uint32),
                                  (c.x.max(0) - lo).view(np.uint32))
        else:
            # the f32 normalisation is within 4u of the f64 one, relative,
            # per component (norm^2, 1 / sqrt and the product round once
            # each); max - min then rounds once more
            x = c.x.astype(np.float64)
            xh = x / np.sqrt((x * x).sum(1, keepdims=True))
            lo, hi = xh.min(0), xh.max(0)
            amax = np.abs(xh).max(0)
            assert (np.abs(vmin - lo) <= 4 * U * amax).all()
            assert (np.abs(vdiff - (hi - lo)) <=
                    8 * U * amax + U * (hi - lo)).all()
        idx.add(c.ids, c.x)
        idx.train(c.x[:100])  # trained: a no-op
        v2, w2 = idx.get_sq_ranges()
        assert np.array_equal(v2, vmin) and np.array_equal(w2, vdiff)
    finally:
        idx.close()
    # without centroids dg_train yields both
    idx = dg.Index(dg.IVF_FLAT, metric, c.d, nlist=c.nlist, storage="sq8")
    try:
        idx.train(c.x)
        assert idx.stats()["is_trained"]
        v3, w3 = idx.get_sq_ranges()
        assert np.array_equal(v3, vmin) and np.array_equal(w3, vdiff)
    finally:
        idx.close()


def test_buffers_and_scan_bytes_shrink():
    c = ir.case_c(L2)
    st = {}
    for storage in ("f32", "sq8"):
        idx = _index(c, storage)
        try:
            idx.search(c.q, 10, nprobe=3)
            assert idx.last_scan_sq8() == (storage == "sq8")
            st[storage] = idx.stats()
        finally:
            idx.close()
    assert st["sq8"]["device_bytes"] < 0.35 * st["f32"]["device_bytes"]
    assert 0 < st["sq8"]["last_scan_bytes_algorithmic"] < \
        0.35 * st["f32"]["last_scan_bytes_algorithmic"]


# --------------------------------------------------------------------------
# scan
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ir.A_METRICS, ids=lambda m: MNAME[m])
@pytest.mark.parametrize("d", h8.A8_DIMS)
def test_d_pipeline(d, metric):
    """Every path of the 64-dim load pipeline (nkp 1..13, partly filled last
    kps included) over a partial wave, a second wave of 4 rows and a second
    chunk of 3 rows, by a full and a partial query tile: k = 10 fused and
    k = N store-all, which reads out every (query, row) pair."""
    _run(ir.case_a(d, metric), ir.run_full_probe, ir.A_K)


@pytest.mark.parametrize(
    "d,metric,nq", h8.B8,
    ids=[f"{d}-{MNAME[m]}-nq{nq}" for d, m, nq in h8.B8])
def test_d_ladder(d, metric, nq):
    """QTM 16 at 2304, 8 at 2305, 4 at 4609 and 8192 (the largest LDS
    images and chunk offsets)."""
    _run(ir.case_b(d, metric, nq), ir.run_full_probe, ir.B_K)


@pytest.mark.parametrize("metric", [L2, IP, COSINE], ids=lambda m: MNAME[m])
def test_edges_partial_probing(metric):
    """Lists of 1, 3, 255..257, 1023..1025 and 2049 rows probed by 1, 8, 9,
    16, 17 and 33 queries; fused and store-all, by k and by size."""
    _run(ir.case_c(metric), ir.run_c)


def test_filters_tombstones_upsert():
    """The upserted rows are re-encoded with the index's ranges; the
    reference after the upsert is taken over what reconstruct returns."""
    _run(ir.case_c(L2), h8.run_d8, reconstruct=True)


@pytest.mark.parametrize("metric", ir.E_METRICS, ids=lambda m: MNAME[m])
def test_range_partial_probing(metric):
    _run(ir.case_e(metric), ir.run_e)


@pytest.mark.parametrize("nq", ir.F_NQS)
def test_graph_replay(nq):
    _run(ir.case_c(L2), ir.run_f, nq)


@pytest.mark.parametrize("metric", [L2, IP, COSINE], ids=lambda m: MNAME[m])
def test_fused_equals_store_all(metric, monkeypatch):
    """One dot-product body: a search that qualifies for both flows returns
    identical ids and bit-identical distances from each."""
    c = ir.case_c(metric)
    idx = _index(c)
    try:
        for nprobe, k in ir.C_FUSED:
            monkeypatch.delenv("DG_SCAN_FUSED", raising=False)
            d1, i1 = idx.search(c.q, k, nprobe=nprobe)
            assert idx.last_scan_fused() and idx.last_scan_sq8()
            monkeypatch.setenv("DG_SCAN_FUSED", "0")
            d0, i0 = idx.search(c.q, k, nprobe=nprobe)
            assert not idx.last_scan_fused() and idx.last_scan_sq8()
            assert np.array_equal(i1, i0), (nprobe, k)
            assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32))
    finally:
        idx.close()


@pytest.mark.parametrize("k", [10, 65])
def test_tiles_over_grid_y_change_nothing(k, monkeypatch):
    """A list's query tiles are strided over grid.y as in the f16 scan (the
    same DG_SCAN_F16_PY switch).  Same ids, same bits, both flows."""
    c = ir.case_c(L2)
    idx = _index(c)
    try:
        got = {}
        for py in ("1", "2", "4", None):
            if py is None:
                monkeypatch.delenv("DG_SCAN_F16_PY", raising=False)
            else:
                monkeypatch.setenv("DG_SCAN_F16_PY", py)
            got[py] = idx.search(c.q, k, nprobe=3)
            assert idx.last_scan_fused() == (k <= 64)
            assert idx.last_scan_sq8()
        for py in ("2", "4", None):
            assert np.array_equal(got[py][1], got["1"][1]), py
            assert np.array_equal(got[py][0].view(np.uint32),
                                  got["1"][0].view(np.uint32)), py
    finally:
        idx.close()


# --------------------------------------------------------------------------
# contract
# --------------------------------------------------------------------------
def test_set_storage_and_range_refusals():
    c = ir.case_a(8, L2)
    vmin, vdiff = h8.ranges_of(c.x)
    idx = dg.Index(dg.IVF_FLAT, L2, c.d, nlist=c.nlist)
    try:
        # ranges belong to SQ8 storage alone
        assert _status(idx.set_sq_ranges, vmin, vdiff) == DG_EINVAL
        assert _status(idx.get_sq_ranges) == DG_EINVAL
        idx.set_storage("sq8")  # untrained and empty
        assert dg.lib().dg_get_storage(idx.h) == 2
        idx.set_sq_ranges(vmin, vdiff)
        idx.set_storage("f16")  # leaving SQ8 drops its ranges
        assert _status(idx.get_sq_ranges) == DG_EINVAL
        idx.set_storage("sq8")
        assert _status(idx.get_sq_ranges) == DG_ENOT_TRAINED
        idx.set_centroids(c.cents)
        for bad_min, bad_diff in ((np.nan, 1.0), (np.inf, 1.0), (0.0, np.nan),
                                  (0.0, np.inf), (0.0, -1e-3)):
            v, w = vmin.copy(), vdiff.copy()
            v[3], w[3] = bad_min, bad_diff
            assert _status(idx.set_sq_ranges, v, w) == DG_EINVAL
        assert _status(idx.get_sq_ranges) == DG_ENOT_TRAINED
        assert _status(idx.add, c.ids, c.x) == DG_ENOT_TRAINED
        w0 = vdiff.copy()
        w0[2] = 0.0  # vdiff = 0 is a valid range
        idx.set_sq_ranges(vmin, w0)
        idx.set_sq_ranges(vmin, vdiff)
        assert idx.storage == "sq8" and idx.stats()["is_trained"]
        idx.add(c.ids, c.x)
        assert _status(idx.set_storage, "f32") == DG_EINVAL
        assert _status(idx.set_storage, "sq8") == DG_EINVAL
        assert _status(idx.set_sq_ranges, vmin, vdiff) == DG_EINVAL
        assert idx.storage == "sq8"
    finally:
        idx.close()
    flat = dg.Index(dg.FLAT, L2, 8)
    try:
        assert _status(flat.set_storage, "sq8") == DG_ENOT_SUPPORT
    finally:
        flat.close()
    assert _status(dg.Index, dg.FLAT, L2, 8, storage="sq8") == DG_ENOT_SUPPORT
    assert _status(dg.Index, dg.IVF_PQ, L2, 16, nlist=4, m=8,
                   storage="sq8") == DG_ENOT_SUPPORT
    assert _status(dg.Index, dg.BINARY_FLAT, dg.HAMMING, 64,
                   storage="sq8") == DG_EINVAL


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_add_refuses_what_is_not_finite(bad):
    c = ir.case_a(12, L2)
    idx = _index(c)
    try:
        n0 = idx.stats()["ntotal"]
        x = c.x[:5].copy()
        x[3, 7] = bad
        new_ids = np.arange(5, dtype=np.int64) + (1 << 20)
        assert _status(idx.add, new_ids, x) == DG_EINVAL
        assert idx.stats()["ntotal"] == n0
        assert _status(idx.reconstruct, new_ids[:1]) == DG_ENOT_FOUND
        x[3, 7] = 1e6  # finite: it saturates
        idx.add(new_ids, x)  # the ids are still free
        assert idx.stats()["ntotal"] == n0 + 5
        vmin, vdiff = idx.get_sq_ranges()
        top = h8.decode(np.array([255]), vmin[7], vdiff[7]).astype(np.float32)
        assert idx.reconstruct(new_ids[3:4])[0, 7] == top[0]
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [L2, COSINE], ids=lambda m: MNAME[m])
def test_refused_upsert_removes_nothing(metric):
    c = ir.case_a(12, L2)
    idx = dg.Index(dg.IVF_FLAT, metric, c.d, nlist=c.nlist, storage="sq8")
    try:
        idx.set_centroids(c.cents)
        rows = h8.normalize_f32(c.x) if metric == COSINE else c.x
        idx.set_sq_ranges(*h8.ranges_of(rows))
        idx.add(c.ids, c.x)
        before = idx.reconstruct(c.ids[:4])
        for bad in (float("nan"), float("inf")):
            x = c.x[:4].copy()
            x[2, 5] = bad
            assert _status(idx.upsert, c.ids[:4], x) == DG_EINVAL
            assert idx.stats()["ntotal"] == c.n
            assert idx.stats()["deleted_count"] == 0
            assert np.array_equal(idx.reconstruct(c.ids[:4]), before)
    finally:
        idx.close()


def test_reserved_arrival_store_follows_the_storage():
    c = ir.case_c(L2)
    st = {}
    for storage in ("f32", "sq8"):
        idx = dg.Index(dg.IVF_FLAT, L2, c.d, nlist=c.nlist, reserve=c.n,
                       storage=storage)
        try:
            idx.set_centroids(c.cents)
            if storage == "sq8":
                idx.set_sq_ranges(*_ranges(c))
            idx.add(c.ids, c.x)
            idx.search(c.q, 10, nprobe=3)
            st[storage] = idx.stats()["device_bytes"]
        finally:
            idx.close()
    assert st["sq8"] < 0.35 * st["f32"]


def test_save_load_round_trip(tmp_path):
    c = ir.case_c(IP)
    idx = _index(c)
    loaded = None
    try:
        p8 = str(tmp_path / "sq8.dgi")
        idx.save(p8)
        assert _status(idx.save_faiss,
                       str(tmp_path / "sq8.faiss")) == DG_ENOT_SUPPORT
        loaded = dg.Index.load(p8)
        assert loaded.storage == "sq8" and loaded.stats()["is_trained"]
        for a, b in zip(idx.get_sq_ranges(), loaded.get_sq_ranges()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        a = idx.reconstruct(c.ids)
        b = loaded.reconstruct(c.ids)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # every list probed: the answer does not depend on the row order
        # inside a list, which a reload may change, except between ties
        d0, i0 = idx.search(c.q, 10, nprobe=c.nlist)
        d1, i1 = loaded.search(c.q, 10, nprobe=c.nlist)
        assert loaded.last_scan_sq8()
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
        untied = np.ones(d0.shape, bool)
        untied[:, 1:] &= d0[:, 1:] != d0[:, :-1]
        untied[:, :-1] &= d0[:, :-1] != d0[:, 1:]
        untied[:, -1] = False
        assert np.array_equal(i0[untied], i1[untied])
        # the container is a quarter of the f32 one, which stays DGI1
        f32 = _index(c, "f32")
        try:
            p32a, p32b = str(tmp_path / "a.dgi"), str(tmp_path / "b.dgi")
            f32.save(p32a)
            f32.save(p32b)
            with open(p32a, "rb") as fa, open(p32b, "rb") as fb:
                ba, bb = fa.read(), fb.read()
            assert ba == bb and ba[:4] == b"1IGD"  # the DGI1 magic, LE
            with open(p8, "rb") as f:
                b8 = f.read()
            assert b8[:4] == b"2IGD" and b8[4:8] == np.int32(2).tobytes()
            assert len(b8) < 0.35 * len(ba)
            back = dg.Index.load(p32a)
            try:
                assert back.storage == "f32"
                assert np.array_equal(back.reconstruct(c.ids), c.x)
            finally:
                back.close()
        finally:
            f32.close()
    finally:
        idx.close()
        if loaded is not None:
            loaded.close()


def test_search_batched_equals_search():
    c = ir.case_c(L2)
    idx = _index(c)
    try:
        d0, i0 = idx.search(c.q[:8], 10, nprobe=3)
        idx.enable_batching()
        d1, i1 = idx.search_batched(c.q[:8], 10, nprobe=3)
        idx.disable_batching()
        assert np.array_equal(i0, i1)
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [L2, IP], ids=lambda m: MNAME[m])
def test_sharded_agrees_with_single(metric):
    c = ir.case_c(metric)
    one = _index(c)
    sh = dg.ShardedIndex(dg.IVF_FLAT, metric, c.d, [0, 0, 0], nlist=c.nlist,
                         storage="sq8")
    try:
        sh.set_centroids(c.cents)
        vmin, vdiff = _ranges(c)
        sh.set_sq_ranges(vmin, vdiff)
        sh.add(c.ids, c.x)
        for i in range(3):
            assert sh.shard(i).storage == "sq8"
            for a, b in zip(sh.shard(i).get_sq_ranges(), (vmin, vdiff)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        stored = one.reconstruct(c.ids)
        ref, b = h8.ref_and_bound8(metric, c.q, stored, vmin, vdiff)
        pos = {int(v): i for i, v in enumerate(c.ids)}
        for k in (10, 65):
            d1, i1 = one.search(c.q, k, nprobe=3)
            ds, is_ = sh.search(c.q, k, nprobe=3)
            assert np.array_equal(i1 < 0, is_ < 0)
            # a row's dot chain and norm do not depend on where the row
            # sits: the same bits, and the same ids wherever untied
            assert np.array_equal(d1.view(np.uint32), ds.view(np.uint32))
            untied = i1 >= 0
            untied[:, 1:] &= d1[:, 1:] != d1[:, :-1]
            untied[:, :-1] &= d1[:, :-1] != d1[:, 1:]
            untied[:, -1] = False
            assert np.array_equal(i1[untied], is_[untied])
            for qi in range(len(c.q)):
                m = int((is_[qi] >= 0).sum())
                rs = np.array([pos[int(v)] for v in is_[qi, :m]], np.int64)
                # distances within b8 of the reference of the row returned
                assert (np.abs(ds[qi, :m] - ref[qi, rs]) <= b[qi, rs]).all()
    finally:
        one.close()
        sh.close()
    with pytest.raises(dg.DgError):
        dg.ShardedIndex(dg.FLAT, L2, 8, [0, 0], storage="sq8")


def test_sharded_train_replicates_the_ranges():
    c = ir.case_c(L2)
    sh = dg.ShardedIndex(dg.IVF_FLAT, L2, c.d, [0, 0, 0], nlist=c.nlist,
                         storage="sq8")
    try:
        sh.train(c.x)
        v0, w0 = sh.get_sq_ranges()
        lo = c.x.min(0)
        assert np.array_equal(v0.view(np.uint32), lo.view(np.uint32))
        assert np.array_equal(w0.view(np.uint32),
                              (c.x.max(0) - lo).view(np.uint32))
        for i in range(3):
            vi, wi = sh.shard(i).get_sq_ranges()
            assert np.array_equal(vi.view(np.uint32), v0.view(np.uint32))
            assert np.array_equal(wi.view(np.uint32), w0.view(np.uint32))
        sh.add(c.ids, c.x)
        ds, is_ = sh.search(c.q, 10, nprobe=c.nlist)
        assert (is_ >= 0).all()
    finally:
        sh.close()


def test_mirror_selftest_sq8():
    assert dg.lib().dg_mirror_selftest_sq8() == 0
