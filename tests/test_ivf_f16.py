"""IVF-Flat with f16 row storage (DG_STORAGE_F16) on the GPU (marked gpu).

Storage: what reconstruct returns is numpy's round-to-nearest-even half of
the input, bit for bit (L2, IP), or of the normalised input within the
derived component bound (COSINE); buffers and algorithmic scan bytes shrink.
Scan: k_ivf_scan_f16 in its fused and its store-all form, every query of
every search held to rules A-D (or the range rules) of flat_reference over
the verified assignment, against the float64 reference over the f32 queries
and the rows the index returns from reconstruct, within the derived bound
b16 (ivf_f16_reference).  The searches are the drivers of ivf_reference,
which test_ivf_f16_cpu.py runs dry.  Contract: the refusals of set_storage,
the finite check of add, save / load, reconstruct, search_batched, the
sharded index and the mirror.
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
import ivf_f16_reference as h16  # noqa: E402
import ivf_reference as ir  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

MNAME = {L2: "L2", IP: "IP", COSINE: "COSINE"}
DG_EINVAL, DG_ENOT_SUPPORT, DG_ENOT_FOUND = 1, 3, 9


@pytest.fixture(scope="module", autouse=True)
def _report_slack():
    yield
    print("\nIVF-Flat f16: largest |dist - ref| / b16 per metric:",
          {MNAME[m]: round(v, 4) for m, v in h16.MAX_RATIO.items()})


@pytest.fixture(autouse=True)
def _default_scan_path(monkeypatch):
    monkeypatch.delenv("DG_SCAN_FUSED", raising=False)


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


def _index(c, storage="f16"):
    idx = dg.Index(dg.IVF_FLAT, c.metric, c.d, nlist=c.nlist,
                   storage=storage)
    idx.set_centroids(c.cents)
    idx.add(c.ids, c.x)
    return idx


class GpuOps16:
    """The driver operations of ivf_reference on an f16 index; the case the
    drivers see carries (ref, b16) over the rows reconstruct returns."""

    def __init__(self, c):
        self.idx = _index(c)
        assert self.idx.storage == "f16"
        self.c = h16.f16_case(c, self.idx.reconstruct(c.ids))
        self.searches = 0

    def verified_assign(self):
        c = self.c
        assign = self.idx.export_assign()
        # rows are assigned from their f32 values, not from the halves
        ir.verify_assign(c.metric, c.x, c.cents, assign,
                         (MNAME[c.metric], c.d))
        assert np.array_equal(np.bincount(assign, minlength=c.nlist), c.lens)
        return assign

    def search(self, where, q, k, nprobe, spec, ref, b, ids, elig, fused):
        gd, gi = self.idx.search(q, k, nprobe=nprobe,
                                 filt=make_dg_filter(spec))
        assert self.idx.last_scan_fused() == fused, where
        assert self.idx.last_scan_f16() and not self.idx.last_scan_pair()
        h16.check_topk(self.c.metric, gd, gi, ref, b, ids, elig, where)
        self.searches += 1

    def range_search(self, where, q, radius, ref, b, ids, elig):
        lims, rd, ri = self.idx.range_search(q, radius)
        assert not self.idx.last_scan_fused() and self.idx.last_scan_f16()
        h16.check_range(self.c.metric, radius, lims, rd, ri, ref, b, ids,
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


def _run(c, driver, *args):
    ops = GpuOps16(c)
    try:
        driver(ops.c, ops.verified_assign(), ops, *args)
        assert ops.searches > 0
    finally:
        ops.close()


# --------------------------------------------------------------------------
# storage
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP], ids=lambda m: MNAME[m])
@pytest.mark.parametrize("d", [5, 32, 100])
def test_reconstruct_is_nearest_even_half(d, metric):
    c = ir.case_a(d, metric)
    x = c.x.copy()
    # ties, the largest finite half, subnormals and values that flush to 0
    x[0, :] = 0.0
    edge = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0,
                     -65504.0, 2.0 ** -25, 3 * 2.0 ** -25, 1e-8, -2.0 ** -14],
                    np.float32)
    x[0, :min(d, 8)] = edge[:min(d, 8)]
    idx = dg.Index(dg.IVF_FLAT, metric, d, nlist=c.nlist, storage="f16")
    try:
        idx.set_centroids(c.cents)
        idx.add(c.ids, x)
        got = idx.reconstruct(c.ids)
        want = x.astype(np.float16)
        assert got.shape == x.shape and got.dtype == np.float32
        assert np.array_equal(got.astype(np.float16).view(np.uint16),
                              want.view(np.uint16))
        assert np.array_equal(got.view(np.uint32),
                              want.astype(np.float32).view(np.uint32))
        # repeated ids, any order
        pick = c.ids[[7, 3, 7, c.n - 1]]
        assert np.array_equal(idx.reconstruct(pick), got[[7, 3, 7, c.n - 1]])
    finally:
        idx.close()


def test_reconstruct_cosine_within_the_component_bound():
    c = ir.case_c(COSINE)
    idx = _index(c)
    try:
        got = idx.reconstruct(c.ids).astype(np.float64)
    finally:
        idx.close()
    x = c.x.astype(np.float64)
    xh = x / np.sqrt((x * x).sum(1, keepdims=True))
    tol = (2.0 ** -11 + 4 * fr.U) * np.abs(xh) + 2.0 ** -25
    assert (np.abs(got - xh) <= tol).all()
    # halves exactly: a second rounding changes nothing
    assert np.array_equal(got.astype(np.float16).astype(np.float64), got)


def test_buffers_and_scan_bytes_shrink():
    c = ir.case_c(L2)
    st = {}
    for storage in ("f32", "f16"):
        idx = _index(c, storage)
        try:
            idx.search(c.q, 10, nprobe=3)
            assert idx.last_scan_f16() == (storage == "f16")
            st[storage] = idx.stats()
        finally:
            idx.close()
    assert st["f16"]["device_bytes"] < 0.6 * st["f32"]["device_bytes"]
    assert 0 < st["f16"]["last_scan_bytes_algorithmic"] < \
        0.6 * st["f32"]["last_scan_bytes_algorithmic"]


# --------------------------------------------------------------------------
# scan
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ir.A_METRICS, ids=lambda m: MNAME[m])
@pytest.mark.parametrize("d", h16.A16_DIMS)
def test_d_pipeline(d, metric):
    """Every path of the 32-dim load pipeline (nkp 1..13, half-empty last
    groups included) over a partial wave, a second wave of 4 rows and a
    second chunk of 3 rows, by a full and a partial query tile: k = 10 fused
    and k = N store-all, which reads out every (query, row) pair."""
    _run(ir.case_a(d, metric), ir.run_full_probe, ir.A_K)


@pytest.mark.parametrize(
    "d,metric,nq", h16.B16_GPU,
    ids=[f"{d}-{MNAME[m]}-nq{nq}" for d, m, nq in h16.B16_GPU])
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
    _run(ir.case_c(L2), h16.run_d16)


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
            assert idx.last_scan_fused() and idx.last_scan_f16()
            monkeypatch.setenv("DG_SCAN_FUSED", "0")
            d0, i0 = idx.search(c.q, k, nprobe=nprobe)
            assert not idx.last_scan_fused() and idx.last_scan_f16()
            assert np.array_equal(i1, i0), (nprobe, k)
            assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32))
    finally:
        idx.close()


@pytest.mark.parametrize("k", [10, 65])
def test_tiles_over_grid_y_change_nothing(k, monkeypatch):
    """A list's query tiles are strided over grid.y (1 per 8 mean probes
    per list, at most 4; here nprobe 3 gives 4).  Lists
    probed by 1 to 33 queries have 1 to 3 tiles: with 1, 2 and 4 block rows
    some rows get no tile, one, or two.  Same ids, same bits, both flows."""
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
        for py in ("2", "4", None):
            assert np.array_equal(got[py][1], got["1"][1]), py
            assert np.array_equal(got[py][0].view(np.uint32),
                                  got["1"][0].view(np.uint32)), py
    finally:
        idx.close()


# --------------------------------------------------------------------------
# contract
# --------------------------------------------------------------------------
def test_set_storage_refusals():
    c = ir.case_a(8, L2)
    idx = dg.Index(dg.IVF_FLAT, L2, c.d, nlist=c.nlist)
    try:
        assert idx.storage == "f32"
        idx.set_storage("f16")  # untrained and empty
        idx.set_centroids(c.cents)
        idx.set_storage("f32")  # trained and empty
        idx.set_storage("f16")
        assert idx.storage == "f16"
        idx.add(c.ids, c.x)
        assert _status(idx.set_storage, "f32") == DG_EINVAL
        assert _status(idx.set_storage, "f16") == DG_EINVAL
        assert idx.storage == "f16"
    finally:
        idx.close()
    flat = dg.Index(dg.FLAT, L2, 8)
    try:
        assert _status(flat.set_storage, "f16") == DG_ENOT_SUPPORT
        flat.set_storage("f32")
    finally:
        flat.close()
    assert _status(dg.Index, dg.FLAT, L2, 8, storage="f16") == DG_ENOT_SUPPORT
    assert _status(dg.Index, dg.IVF_PQ, L2, 16, nlist=4, m=8,
                   storage="f16") == DG_ENOT_SUPPORT
    assert _status(dg.Index, dg.BINARY_FLAT, dg.HAMMING, 64,
                   storage="f16") == DG_EINVAL
    assert dg.lib().dg_get_storage(None) == -1


@pytest.mark.parametrize("bad", [70000.0, -65520.0, float("nan"),
                                 float("inf")])
def test_add_refuses_what_no_half_holds(bad):
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
        idx.add(new_ids, c.x[:5])  # the ids are still free
        assert idx.stats()["ntotal"] == n0 + 5
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [L2, COSINE], ids=lambda m: MNAME[m])
def test_refused_upsert_removes_nothing(metric):
    c = ir.case_a(12, metric if metric != COSINE else L2)
    idx = dg.Index(dg.IVF_FLAT, metric, c.d, nlist=c.nlist, storage="f16")
    try:
        idx.set_centroids(c.cents)
        idx.add(c.ids, c.x)
        before = idx.reconstruct(c.ids[:4])
        x = c.x[:4].copy()
        x[2, 5] = float("nan")
        assert _status(idx.upsert, c.ids[:4], x) == DG_EINVAL
        x[2, 5] = 70000.0
        if metric == COSINE:  # normalised before it is stored: it fits
            idx.upsert(c.ids[:4], x)
            assert idx.stats()["ntotal"] == c.n
        else:
            assert _status(idx.upsert, c.ids[:4], x) == DG_EINVAL
            assert idx.stats()["ntotal"] == c.n
            assert idx.stats()["deleted_count"] == 0
            assert np.array_equal(idx.reconstruct(c.ids[:4]), before)
    finally:
        idx.close()


def test_reserved_arrival_store_follows_the_storage():
    c = ir.case_c(L2)
    st = {}
    for storage in ("f32", "f16"):
        idx = dg.Index(dg.IVF_FLAT, L2, c.d, nlist=c.nlist, reserve=c.n,
                       storage=storage)
        try:
            idx.set_centroids(c.cents)
            idx.add(c.ids, c.x)
            idx.search(c.q, 10, nprobe=3)
            st[storage] = idx.stats()["device_bytes"]
        finally:
            idx.close()
    assert st["f16"] < 0.6 * st["f32"]


def test_save_load_round_trip(tmp_path):
    c = ir.case_c(IP)
    idx = _index(c)
    loaded = None
    try:
        p16 = str(tmp_path / "f16.dgi")
        idx.save(p16)
        assert _status(idx.save_faiss,
                       str(tmp_path / "f16.faiss")) == DG_ENOT_SUPPORT
        loaded = dg.Index.load(p16)
        assert loaded.storage == "f16"
        a = idx.reconstruct(c.ids)
        b = loaded.reconstruct(c.ids)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        # every list probed: the answer does not depend on the row order
        # inside a list, which a reload may change, except between ties
        d0, i0 = idx.search(c.q, 10, nprobe=c.nlist)
        d1, i1 = loaded.search(c.q, 10, nprobe=c.nlist)
        assert loaded.last_scan_f16()
        assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
        untied = np.ones(d0.shape, bool)
        untied[:, 1:] &= d0[:, 1:] != d0[:, :-1]
        untied[:, :-1] &= d0[:, :-1] != d0[:, 1:]
        untied[:, -1] = False
        assert np.array_equal(i0[untied], i1[untied])
        # the container is half the size of the f32 one
        f32 = _index(c, "f32")
        try:
            p32a, p32b = str(tmp_path / "a.dgi"), str(tmp_path / "b.dgi")
            f32.save(p32a)
            f32.save(p32b)
            with open(p32a, "rb") as fa, open(p32b, "rb") as fb:
                ba, bb = fa.read(), fb.read()
            assert ba == bb and ba[:4] == b"1IGD"  # the DGI1 magic, LE
            with open(p16, "rb") as f:
                b16 = f.read()
            assert b16[:4] == b"2IGD" and len(b16) < 0.6 * len(ba)
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


def test_reconstruct_contract():
    c = ir.case_a(13, L2)
    idx = _index(c)
    flat = dg.Index(dg.FLAT, L2, c.d)
    f32 = _index(c, "f32")
    try:
        idx.remove(c.ids[[4]])
        l = dg.lib()
        for ids in (c.ids[[1, 4]], np.array([c.ids[1], 12], np.int64)):
            out = np.full((2, c.d), -7.0, np.float32)
            assert l.dg_reconstruct(idx.h, 2, ids, out) == DG_ENOT_FOUND
            assert (out == -7.0).all()
        assert np.array_equal(
            idx.reconstruct(c.ids[[1]]),
            c.x[[1]].astype(np.float16).astype(np.float32))
        # f32 storage returns the input bits, FLAT and IVF
        flat.add(c.ids, c.x)
        for ix in (flat, f32):
            assert np.array_equal(ix.reconstruct(c.ids).view(np.uint32),
                                  c.x.view(np.uint32))
    finally:
        idx.close()
        flat.close()
        f32.close()
    pq = dg.Index(dg.IVF_PQ, L2, 16, nlist=4, m=8)
    try:
        assert _status(pq.reconstruct, np.array([1], np.int64)) == \
            DG_ENOT_SUPPORT
    finally:
        pq.close()
    bn = dg.Index(dg.BINARY_FLAT, dg.HAMMING, 64)
    try:
        out = np.zeros((1, 64), np.float32)
        assert dg.lib().dg_reconstruct(bn.h, 1, np.array([1], np.int64),
                                       out) == DG_EINVAL
    finally:
        bn.close()


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
                         storage="f16")
    try:
        sh.set_centroids(c.cents)
        sh.add(c.ids, c.x)
        for i in range(3):
            assert sh.shard(i).storage == "f16"
        stored = one.reconstruct(c.ids)
        ref, b = h16.ref_and_bound16(metric, c.q, stored)
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
                # distances within b16 of the reference of the row returned
                assert (np.abs(ds[qi, :m] - ref[qi, rs]) <= b[qi, rs]).all()
    finally:
        one.close()
        sh.close()
    with pytest.raises(dg.DgError):
        dg.ShardedIndex(dg.FLAT, L2, 8, [0, 0], storage="f16")


def test_mirror_selftest_f16():
    assert dg.lib().dg_mirror_selftest_f16() == 0
