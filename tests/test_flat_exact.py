"""Flat exact search, float range search and the float filters against the
float64 reference of flat_reference.py (marked gpu).

The path under test is sgemm_dots -> k_dots_mfma or rocBLAS ->
k_select_dense -> k_select_u64 -> k_emit, the dense and candidate range
kernels, and the row pass bitmap that the filters and tombstones feed.
Reference, bound and the acceptance rules A-D / range rules are documented
in flat_reference.py; every query of every search is checked, and each case
first asserts on the reference alone that the bound is tight enough for the
checks to mean something.

Geometry the shapes rest on:
  - GEMM route (sgemm_dots, over the dimension padded to a multiple of 4):
    the hand MFMA kernel for rows <= 8, or for rows >= 48 and
    64 <= cols <= 16384 and d >= 64; rocBLAS otherwise.  The hand kernel
    works in 128 x 128 x 32 tiles.
  - With k = N a Flat search returns every element of the dots matrix, so
    check A covers the whole GEMM output.
  - The dense select runs 8 column segments of ceil(N / 8) for N <= 65536,
    merged by k_select_u64; the block shrinks to 16 threads at k = 300 and
    to 4 at k = 2048, the largest k the library takes.
  - Flat splits the rows into chunks when N > max(65536, 2^29 / nq).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO, os.path.join(REPO, "dingo-store_amd")]

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")
import flat_reference as fr  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

assert (dg.L2, dg.IP, dg.COSINE) == (L2, IP, COSINE)
MNAME = {L2: "L2", IP: "IP", COSINE: "COSINE"}


@pytest.fixture(scope="module", autouse=True)
def _report_slack():
    yield
    print("\nlargest |dist - ref| / b per metric:",
          {MNAME[m]: round(v, 4) for m, v in fr.MAX_RATIO.items()})


def flat_index(metric, x, ids=None):
    idx = dg.Index(dg.FLAT, metric, x.shape[1])
    idx.add(np.arange(len(x), dtype=np.int64) if ids is None else ids, x)
    return idx


def ivf_index(metric, x, ids, nlist=8):
    """IVF-Flat whose centroids are the first nlist rows; searched with
    nprobe = nlist, so eligible = admissible."""
    idx = dg.Index(dg.IVF_FLAT, metric, x.shape[1], nlist=nlist)
    idx.set_centroids(x[:nlist].copy())
    idx.add(ids, x)
    return idx


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


def search_and_check(idx, metric, q, k, ref, b, ids, elig, where,
                     nprobe=0, spec=None):
    fr.assert_topk_strength(metric, ref, b, elig, k, where)
    gd, gi = idx.search(q, k, nprobe=nprobe, filt=make_dg_filter(spec))
    return fr.check_topk(metric, gd, gi, ref, b, ids, elig, where)


# --------------------------------------------------------------------------
# a. GEMM tile edges, read out completely (k = N)
# --------------------------------------------------------------------------
def _full_readout(metric, nq, n, d):
    q, x = fr.gaussian(fr.gemm_seed(nq, n, d), nq, n, d, metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    idx = flat_index(metric, x)
    try:
        search_and_check(idx, metric, q, n, ref, b, np.arange(n),
                         np.ones(n, bool), (MNAME[metric], nq, n, d))
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("shape", fr.GEMM_TILE_SHAPES, ids=str)
def test_gemm_mfma_tile_edges(shape, metric):
    _full_readout(metric, *shape)


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("shape", fr.GEMM_LATENCY_SHAPES, ids=str)
def test_gemm_mfma_latency_route(shape, metric):
    _full_readout(metric, *shape)


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("shape", fr.GEMM_ROCBLAS_SHAPES, ids=str)
def test_gemm_rocblas_route(shape, metric):
    _full_readout(metric, *shape)


@pytest.mark.parametrize("shape", fr.GEMM_COSINE_SHAPES, ids=str)
def test_gemm_cosine(shape):
    _full_readout(COSINE, *shape)


# --------------------------------------------------------------------------
# b. selector edges
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("n", sorted({n for n, _ in fr.SELECT_SMALL}))
def test_select_segment_edges(n, metric):
    q, x = fr.gaussian(fr.select_seed(n), 4, n, fr.SELECT_D, metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    idx = flat_index(metric, x)
    try:
        for k in [k for m, k in fr.SELECT_SMALL if m == n]:
            search_and_check(idx, metric, q, k, ref, b, np.arange(n),
                             np.ones(n, bool), (MNAME[metric], n, k))
        if n > 2048:  # k = N is beyond the library's cap: a loud error
            with pytest.raises(dg.DgError):
                idx.search(q, n)
    finally:
        idx.close()


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("n,k", fr.SELECT_WIDE)
def test_select_wide_k(n, k, metric):
    q, x = fr.gaussian(fr.select_seed(n), 2, n, fr.SELECT_D, metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    idx = flat_index(metric, x)
    try:
        search_and_check(idx, metric, q, k, ref, b, np.arange(n),
                         np.ones(n, bool), (MNAME[metric], n, k))
    finally:
        idx.close()


@pytest.mark.parametrize("nq", [4, 64])
def test_select_exact_duplicates(nq):
    q, x, dup = fr.duplicates_case(nq)
    n = len(x)
    ids = 100 + 2 * np.arange(n, dtype=np.int64)  # ascending with arrival
    ref, b = fr.ref_and_bound(L2, q, x)
    idx = flat_index(L2, x, ids)
    try:
        fr.assert_topk_strength(L2, ref, b, np.ones(n, bool), 10)
        gd, gi = idx.search(q, 10)
        fr.check_topk(L2, gd, gi, ref, b, ids, np.ones(n, bool), nq)
    finally:
        idx.close()
    for qi in range(nq):
        # the copies are the six best rows by more than the bounds
        others = np.delete(ref[qi], dup)
        assert ref[qi, dup[0]] + 2 * b[qi].max() < others.min() - \
            2 * b[qi].max()
        assert set(gi[qi, :6]) == set(ids[dup]), (qi, gi[qi])
        if nq <= 8:
            # one kernel, one summation order: equal keys, and pack_cand
            # orders equal keys by row
            assert (gd[qi, :6] == gd[qi, 0]).all(), (qi, gd[qi, :6])
            assert np.array_equal(gi[qi, :6], ids[dup]), (qi, gi[qi])
        else:
            assert gd[qi, 5] - gd[qi, 0] <= 2 * b[qi, dup[0]], (qi, gd[qi])


# --------------------------------------------------------------------------
# c. multi-chunk Flat
# --------------------------------------------------------------------------
def _check_all_rows_cd(metric, gd, gi, n_elig, known_ids):
    """C and D for every query (no reference): k distinct known ids, no
    padding, monotone distances."""
    k = gi.shape[1]
    assert n_elig >= k
    assert (gi >= 0).all() and np.isin(gi, known_ids).all()
    srt = np.sort(gi, axis=1)
    assert (np.diff(srt, axis=1) > 0).all(), "duplicate ids in a row"
    assert (np.diff(fr.better_sign(metric) * gd, axis=1) >= 0).all()


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_multichunk_flat(metric):
    q, x = fr.multichunk_data(metric)
    n = fr.MC_N
    assert n > max(65536, (1 << 29) // fr.MC_NQ)  # two chunks: 65536 + 64
    rows = fr.multichunk_samples()
    ref, b = fr.ref_and_bound(metric, q[rows], x)
    ids = np.arange(n, dtype=np.int64)
    elig = np.ones(n, bool)
    idx = flat_index(metric, x)
    try:
        for removed in (False, True):
            if removed:
                victims = fr.multichunk_victims(metric, ref)
                assert (victims < fr.MC_CHUNK).sum() == 3
                assert (victims >= fr.MC_CHUNK).sum() == 3
                idx.remove(ids[victims])
                elig[victims] = False
                assert elig.sum() > 65536
            fr.assert_topk_strength(metric, ref, b, elig, fr.MC_K)
            gd, gi = idx.search(q, fr.MC_K)
            fr.check_topk(metric, gd[rows], gi[rows], ref, b, ids, elig,
                          (MNAME[metric], "removed", removed))
            _check_all_rows_cd(metric, gd, gi, int(elig.sum()), ids[elig])
            if removed:
                assert not np.isin(gi, ids[victims]).any()
        # range search on the same (two-chunk, six rows removed) index
        radius = fr.kth_radius(metric, ref, elig, 5)
        fr.assert_range_strength(metric, [radius], ref, b, elig)
        lims, rd, ri = idx.range_search(q, radius)
        fr.check_range(metric, radius, lims, rd, ri, ref, b, ids, elig,
                       MNAME[metric], queries=rows)
        assert not np.isin(ri, ids[~elig]).any()
        bad = ~(rd < np.float32(radius)) if metric == L2 else \
            ~(rd > np.float32(radius))
        assert not bad.any(), (ri[bad], rd[bad])
    finally:
        idx.close()


# --------------------------------------------------------------------------
# d. filters on float indexes
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filt_data():
    q, x = fr.gaussian(fr.FILT_SEED, fr.FILT_NQ, fr.FILT_N, fr.FILT_D, L2)
    ref, b = fr.ref_and_bound(L2, q, x)
    return q, x, fr.filter_ids(), ref, b, fr.filter_specs()


def _filter_matrix(idx, filt_data, ks, nprobe):
    q, x, ids, ref, b, specs = filt_data
    alive = np.ones(len(ids), bool)
    for removed in (False, True):
        if removed:
            victims = fr.filter_victims()
            idx.remove(ids[victims])
            alive[victims] = False
        for name, spec in specs.items():
            adm = fr.filter_mask(spec, ids)
            if removed:  # the pass removes admissible rows of every kind
                assert (adm & ~alive).any() or name == "range_empty", name
            elig = alive & adm
            for k in ks:
                search_and_check(idx, L2, q, k, ref, b, ids, elig,
                                 (name, k, "removed", removed),
                                 nprobe=nprobe, spec=spec)
            if name == "range_empty":
                gd, gi = idx.search(q, 10, nprobe=nprobe,
                                    filt=make_dg_filter(spec))
                assert (gi == -1).all() and (gd == 0.0).all()
            if name == "sorted_few":
                assert 0 < elig.sum() < min(ks)
        # no filter, tombstones only
        for k in ks:
            search_and_check(idx, L2, q, k, ref, b, ids, alive,
                             ("none", k, "removed", removed), nprobe=nprobe)


def test_filters_flat(filt_data):
    q, x, ids, ref, b, specs = filt_data
    idx = flat_index(L2, x, ids)
    try:
        _filter_matrix(idx, filt_data, (10,), 0)
    finally:
        idx.close()


def test_filters_ivfflat(filt_data):
    """k = 10 runs the fused per-wave top-k scan, k = 200 the scan that
    stores every candidate."""
    q, x, ids, ref, b, specs = filt_data
    idx = ivf_index(L2, x, ids)
    try:
        gd, gi = idx.search(q, 10, nprobe=8)
        assert idx.last_scan_fused()
        gd, gi = idx.search(q, 200, nprobe=8)
        assert not idx.last_scan_fused()
        _filter_matrix(idx, filt_data, (10, 200), 8)
    finally:
        idx.close()


def test_filters_range_search_flat(filt_data):
    q, x, ids, ref, b, specs = filt_data
    idx = flat_index(L2, x, ids)
    try:
        for name, spec in specs.items():
            elig = fr.filter_mask(spec, ids)
            if elig.sum() > 20:
                radius = fr.kth_radius(L2, ref, elig, 5)
                fr.assert_range_strength(L2, [radius], ref, b, elig, name)
            else:  # all of a handful, or of nothing
                radius = float(np.float32(ref.max() * 2))
            lims, rd, ri = idx.range_search(q, radius,
                                            filt=make_dg_filter(spec))
            fr.check_range(L2, radius, lims, rd, ri, ref, b, ids, elig, name)
            if elig.sum() <= 20:
                assert (np.diff(lims) == elig.sum()).all(), name
    finally:
        idx.close()


# --------------------------------------------------------------------------
# e. range search semantics
# --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[L2, IP, COSINE],
                ids=["L2", "IP", "COSINE"])
def range_data(request):
    metric = request.param
    q, x = fr.gaussian(fr.FILT_SEED, fr.FILT_NQ, fr.FILT_N, fr.FILT_D,
                       metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    qs = x[fr.self_query_rows()].copy()
    sref, sb = fr.ref_and_bound(metric, qs, x)
    return metric, q, x, fr.filter_ids(), ref, b, qs, sref, sb


def _make(kind, metric, x, ids):
    return flat_index(metric, x, ids) if kind == "flat" else \
        ivf_index(metric, x, ids)


@pytest.mark.parametrize("kind", ["flat", "ivfflat"])
def test_range_reference_radii(range_data, kind):
    metric, q, x, ids, ref, b, qs, sref, sb = range_data
    elig = np.ones(len(ids), bool)
    radii = fr.range_radii(metric, ref, elig)
    fr.assert_range_strength(metric, radii, ref, b, elig)
    idx = _make(kind, metric, x, ids)
    try:
        sizes = []
        for radius in radii:
            lims, rd, ri = idx.range_search(q, radius)
            fr.check_range(metric, radius, lims, rd, ri, ref, b, ids, elig,
                           (kind, MNAME[metric]))
            sizes.append(np.diff(lims))
        assert (sizes[0] > 0).any() and (sizes[0] < len(ids)).all()
        assert (sizes[1] == 0).all()
        assert (sizes[2] == len(ids)).all()
    finally:
        idx.close()


@pytest.mark.parametrize("kind", ["flat", "ivfflat"])
def test_range_radius_on_returned_value(range_data, kind):
    """Radii that are float32 distances the index itself returned: the row
    that produced the value sits exactly on the boundary, where an admission
    test and an emitted distance that round differently disagree."""
    metric, q, x, ids, ref, b, qs, sref, sb = range_data
    elig = np.ones(len(ids), bool)
    idx = _make(kind, metric, x, ids)
    try:
        gd, gi = idx.search(q, 40, nprobe=8)
        fr.check_topk(metric, gd, gi, ref, b, ids, elig, kind)
        radii = np.unique(gd[:, [4, 39]])
        fr.assert_range_strength(metric, radii, ref, b, elig)
        for radius in radii:
            lims, rd, ri = idx.range_search(q, float(radius))
            fr.check_range(metric, float(radius), lims, rd, ri, ref, b, ids,
                           elig, (kind, MNAME[metric]))
    finally:
        idx.close()


@pytest.mark.parametrize("kind", ["flat", "ivfflat"])
def test_range_self_queries_zero_and_negative_radius(range_data, kind):
    """Queries equal to stored rows.  L2: dist < 0 and dist < -1 have no
    solution, the clamped self distance 0.0 included.  IP / COSINE: the
    reference radii, which put the self match (the best score) inside."""
    metric, q, x, ids, ref, b, qs, sref, sb = range_data
    elig = np.ones(len(ids), bool)
    idx = _make(kind, metric, x, ids)
    try:
        radii = fr.range_radii(metric, sref, elig) + [0.0, -1.0]
        fr.assert_range_strength(metric, radii, sref, sb, elig)
        for radius in radii:
            lims, rd, ri = idx.range_search(qs, radius)
            fr.check_range(metric, radius, lims, rd, ri, sref, sb, ids, elig,
                           (kind, MNAME[metric]))
            if metric == L2 and radius <= 0.0:
                assert lims[-1] == 0, (radius, ri, rd)
    finally:
        idx.close()
