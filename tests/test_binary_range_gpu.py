"""Range search of the binary (Hamming) Flat and IVF-Flat indexes on the GPU
(marked gpu).

Reference: the numpy Hamming oracle in hamming_oracle.py.  A row must be
returned iff it is admissible (not removed, passes the filter, and for IVF
lies in a probed list) and hamming(query, row) < radius, strictly.
Distances are integers, so every check is exact: the returned (id, distance)
pairs of every query equal the oracle's set, in (distance, id) ascending
order, and lims is the running count.  IVF list membership is taken from
export_assign(); the probed lists are recomputed by (distance, list id).

The dataset is the one of test_binary_gpu.py (same generator and seeds,
rebuilt here), so the shapes sit on the same kernel edges: N = 5893 =
23 * 256 + 5 columns, nq = 110 = 3 * 32 + 14 queries for the 256 x 32 tile
of the Flat range kernel, and d = 2056 adds 65 words: two full 32-word LDS
tiles plus one word.
"""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "dingo-store_amd")]

import hamming_oracle as ho  # noqa: E402

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")

DG_EINVAL, DG_ENOT_SUPPORT = 1, 3
DIMS = [8, 40, 256, 1000, 2056]
LENS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 2049]
NLIST = len(LENS)
N = sum(LENS)
QPL = [1, 8, 9, 16, 17, 33, 1, 8, 17]
NQ = sum(QPL)
NPROBES = [1, 3, NLIST]
# Flat hits at the partial radius, counted on the CPU with this generator
FLAT_TOTALS = {8: 79574, 40: 39202, 256: 36897, 1000: 40451}
FLAT_LARGEST = {8: 1937, 40: 1783, 256: 1701, 1000: 1973}


def partial_radius(d):
    return max(2, round(0.095 * d))


def radii(d):
    return [0, partial_radius(d), d // 2, d + 1]


class Data:
    pass


@functools.lru_cache(maxsize=None)
def dataset(d):
    """Prototype codes as injected centroids; base rows and queries are a
    prototype with 5 % of the bits flipped.  Computed once per d and never
    modified."""
    rng = np.random.default_rng(1000 + d)
    t = Data()
    t.d = d
    t.protos = rng.integers(0, 256, (NLIST, d // 8), dtype=np.uint8)
    t.base = ho.flip_bits(t.protos[np.repeat(np.arange(NLIST), LENS)], 0.05,
                          rng)
    t.ids = np.arange(N, dtype=np.int64) * 3 + 7
    t.queries = ho.flip_bits(t.protos[np.repeat(np.arange(NLIST), QPL)],
                             0.05, rng)
    t.dist = ho.hamming(t.queries, t.base)        # [nq, N]
    t.coarse = ho.hamming(t.queries, t.protos)    # [nq, NLIST]
    t.assign = ho.hamming(t.base, t.protos).argmin(axis=1).astype(np.int32)
    for a in (t.protos, t.base, t.ids, t.queries, t.dist, t.coarse, t.assign):
        a.setflags(write=False)
    return t


def make_index(kind, t):
    idx = dg.Index(kind, dg.HAMMING, t.d, nlist=NLIST)
    if kind == dg.BINARY_IVF_FLAT:
        idx.set_centroids(t.protos)
    idx.add(t.ids, t.base)
    return idx


def admissible(row_ok, assign=None, probed=None, nq=NQ):
    """[nq, n] mask: row_ok and, for IVF, the row's list is probed."""
    adm = np.broadcast_to(row_ok, (nq, len(row_ok)))
    if assign is not None:
        lut = np.zeros((nq, NLIST), bool)
        np.put_along_axis(lut, probed, True, axis=1)
        adm = adm & lut[:, assign]
    return adm


def expected(dist, row_ids, adm, radius):
    """The oracle's CSR answer: per query the admissible rows strictly below
    the radius, ascending by (distance, id)."""
    hit = adm & (dist < radius)
    q, r = np.nonzero(hit)
    order = np.lexsort((row_ids[r], dist[q, r], q))
    q, r = q[order], r[order]
    lims = np.zeros(dist.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(q, minlength=dist.shape[0]), out=lims[1:])
    return lims, dist[q, r].astype(np.float32), row_ids[r]


def check(got, dist, row_ids, adm, radius, where):
    lims, gd, gi = got
    elims, ed, ei = expected(dist, row_ids, adm, radius)
    print(f"{where}: radius={radius} total hits={int(elims[-1])} "
          f"(got {int(lims[-1])}) empty queries="
          f"{int((np.diff(elims) == 0).sum())} largest query="
          f"{int(np.diff(elims).max())}")
    assert lims.dtype == np.int64 and lims[0] == 0
    assert np.array_equal(lims, elims), where
    assert gd.dtype == np.float32 and gi.dtype == np.int64
    assert np.array_equal(gi, ei), where
    assert gd.tobytes() == ed.tobytes(), where
    return elims


# ---------------- geometry sweep ----------------
@pytest.mark.parametrize("d", DIMS)
def test_flat_geometry_sweep(d):
    t = dataset(d)
    idx = make_index(dg.BINARY_FLAT, t)
    adm = admissible(np.ones(N, bool))
    for radius in radii(d):
        got = idx.range_search_binary(t.queries, radius)
        elims = check(got, t.dist, t.ids, adm, radius, f"flat d={d}")
        if radius == 0:
            assert elims[-1] == 0
        if radius == d + 1:
            assert (np.diff(elims) == N).all()
        if radius == partial_radius(d) and d in FLAT_TOTALS:
            # the generator produces the documented workload
            assert elims[-1] == FLAT_TOTALS[d]
            assert np.diff(elims).max() == FLAT_LARGEST[d]
    # nprobe is ignored by Flat
    a = idx.range_search_binary(t.queries, partial_radius(d), nprobe=1)
    check(a, t.dist, t.ids, adm, partial_radius(d), f"flat d={d} nprobe=1")
    idx.close()


@pytest.mark.parametrize("d", DIMS)
def test_ivf_geometry_sweep(d):
    t = dataset(d)
    idx = make_index(dg.BINARY_IVF_FLAT, t)
    assign = idx.export_assign()
    assert np.array_equal(assign, t.assign)
    for nprobe in NPROBES:
        adm = admissible(np.ones(N, bool), assign,
                         ho.probed_lists(t.coarse, nprobe))
        for radius in radii(d):
            got = idx.range_search_binary(t.queries, radius, nprobe=nprobe)
            check(got, t.dist, t.ids, adm, radius,
                  f"ivf d={d} nprobe={nprobe}")
    # nprobe <= 0 defaults to 80, clamped to nlist; larger values clamp too
    adm = admissible(np.ones(N, bool), assign,
                     ho.probed_lists(t.coarse, NLIST))
    for nprobe in (0, -3, NLIST + 5):
        got = idx.range_search_binary(t.queries, partial_radius(d),
                                      nprobe=nprobe)
        check(got, t.dist, t.ids, adm, partial_radius(d),
              f"ivf d={d} nprobe={nprobe}")
    idx.close()


def test_flat_columns_in_several_launches(monkeypatch):
    """The Flat range kernel covers the columns in spans when one launch
    would exceed its block limit (2^30, above 33M rows at a full query
    batch).  DG_RANGE_SPAN_BLOCKS lowers the limit: with 4 query tiles, 8
    blocks per launch make spans of 512 columns, 12 launches for N = 5893
    with a last span of 261 columns, and 1 block (less than one column tile
    per query tile) falls back to spans of 256.  Rows of the later spans
    must come back with their own ids, bitmap bits and lims slots: same
    bytes as the single launch, with a filter and tombstones in play."""
    t = dataset(256)
    idx = make_index(dg.BINARY_FLAT, t)
    gone = np.arange(3, N, 11)
    idx.remove(t.ids[gone])
    alive = np.ones(N, bool)
    alive[gone] = False
    lo, hi = int(t.ids[N // 5]), int(t.ids[4 * N // 5])
    filt = dg.make_filter(1, False, min_id=lo, max_id=hi)
    ok = alive & (t.ids >= lo) & (t.ids < hi)
    adm = admissible(ok)
    for radius in (partial_radius(256), 128, 257):
        monkeypatch.delenv("DG_RANGE_SPAN_BLOCKS", raising=False)
        one = idx.range_search_binary(t.queries, radius, filt=filt)
        check(one, t.dist, t.ids, adm, radius, "one launch")
        for blocks in ("8", "1"):
            monkeypatch.setenv("DG_RANGE_SPAN_BLOCKS", blocks)
            got = idx.range_search_binary(t.queries, radius, filt=filt)
            check(got, t.dist, t.ids, adm, radius, f"span blocks={blocks}")
            for x, y in zip(one, got):
                assert x.tobytes() == y.tobytes()
    idx.close()


# ---------------- smallest shapes ----------------
@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
@pytest.mark.parametrize("n,nq", [(1, 1), (255, 33)])
def test_smallest_shapes(kind, n, nq):
    t = dataset(40)
    idx = dg.Index(kind, dg.HAMMING, 40, nlist=NLIST)
    if kind == dg.BINARY_IVF_FLAT:
        idx.set_centroids(t.protos)
    rows = np.arange(N - n, N)  # the tail: rows of the last list
    idx.add(t.ids[rows], t.base[rows])
    q = t.queries[NQ - nq:]
    dist = t.dist[NQ - nq:][:, rows]
    assign = probed = None
    if kind == dg.BINARY_IVF_FLAT:
        assign = idx.export_assign()
        assert np.array_equal(assign, t.assign[rows])
        probed = ho.probed_lists(t.coarse[NQ - nq:], 3)
    adm = admissible(np.ones(n, bool), assign, probed, nq=nq)
    for radius in radii(40):
        got = idx.range_search_binary(q, radius, nprobe=3)
        check(got, dist, t.ids[rows], adm, radius, f"n={n} nq={nq}")
    idx.close()


@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_empty_and_untrained(kind):
    """An empty index, and an IVF index without centroids, return all-zero
    lims with DG_OK."""
    t = dataset(40)
    idx = dg.Index(kind, dg.HAMMING, 40, nlist=NLIST)
    if kind == dg.BINARY_IVF_FLAT:
        assert idx.stats()["is_trained"] == 0
        lims, gd, gi = idx.range_search_binary(t.queries[:5], 41, nprobe=3)
        assert (lims == 0).all() and len(gd) == 0 and len(gi) == 0
        idx.set_centroids(t.protos)
    lims, gd, gi = idx.range_search_binary(t.queries[:5], 41)
    assert lims.shape == (6,) and (lims == 0).all()
    assert len(gd) == 0 and len(gi) == 0
    idx.close()


# ---------------- filters, tombstones, upsert ----------------
def _filters(t):
    rng = np.random.default_rng(77)
    lo, hi = int(t.ids[N // 4]), int(t.ids[3 * N // 4])
    subset = np.sort(rng.choice(t.ids, N // 3, replace=False))
    with_missing = np.sort(np.concatenate([subset, [1, 2, int(t.ids[-1]) + 5]]))
    base = 7
    nbits = 64 * ((2 * int(t.ids[-1]) // 3) // 64)  # ids past nbits exist
    bits = rng.random(nbits) < 0.5
    bitmap = np.packbits(bits, bitorder="little").view(np.uint64)
    rel = t.ids - base
    in_bm = (rel >= 0) & (rel < nbits) & bits[np.clip(rel, 0, nbits - 1)]
    cases = []
    for neg in (False, True):
        cases.append((f"range neg={neg}",
                      dg.make_filter(1, neg, min_id=lo, max_id=hi),
                      ((t.ids >= lo) & (t.ids < hi)) ^ neg))
        cases.append((f"sorted neg={neg}",
                      dg.make_filter(2, neg, ids=with_missing),
                      np.isin(t.ids, subset) ^ neg))
        cases.append((f"bitmap neg={neg}",
                      dg.make_filter(3, neg, bitmap=bitmap, bitmap_base=base),
                      in_bm ^ neg))
    return cases


@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_filters(kind):
    t = dataset(256)
    idx = make_index(kind, t)
    ivf = kind == dg.BINARY_IVF_FLAT
    probed = ho.probed_lists(t.coarse, 3)
    radius = partial_radius(256)
    for name, filt, ok in _filters(t):
        assert 0 < ok.sum() < N, name
        adm = admissible(ok, t.assign if ivf else None,
                         probed if ivf else None)
        got = idx.range_search_binary(t.queries, radius, nprobe=3, filt=filt)
        check(got, t.dist, t.ids, adm, radius, name)
    idx.close()


@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_remove_and_upsert(kind):
    t = dataset(256)
    idx = make_index(kind, t)
    ivf = kind == dg.BINARY_IVF_FLAT
    rng = np.random.default_rng(5)
    probed = ho.probed_lists(t.coarse, 3)
    radius = partial_radius(256)

    gone = rng.choice(N, N // 10, replace=False)
    idx.remove(t.ids[gone])
    alive = np.ones(N, bool)
    alive[gone] = False
    adm = admissible(alive, t.assign if ivf else None,
                     probed if ivf else None)
    got = idx.range_search_binary(t.queries, radius, nprobe=3)
    check(got, t.dist, t.ids, adm, radius, "after remove")
    # tombstones and a filter together
    name, filt, ok = _filters(t)[1]
    adm = admissible(alive & ok, t.assign if ivf else None,
                     probed if ivf else None)
    got = idx.range_search_binary(t.queries, radius, nprobe=3, filt=filt)
    check(got, t.dist, t.ids, adm, radius, "after remove, " + name)

    # upsert: live rows with changed bits, removed rows coming back, new ids
    live_rows = np.nonzero(alive)[0]
    up_rows = np.concatenate([rng.choice(live_rows, 40, replace=False),
                              gone[:10]])
    up_ids = np.concatenate([t.ids[up_rows], [900001, 900002, 900003]])
    up_codes = ho.flip_bits(
        t.base[np.concatenate([up_rows, [0, 300, 5000]])], 0.02, rng)
    idx.upsert(up_ids, up_codes)
    rows = np.concatenate([t.base, up_codes])
    row_ids = np.concatenate([t.ids, up_ids])
    ok = np.concatenate([alive & ~np.isin(t.ids, up_ids),
                         np.ones(len(up_ids), bool)])
    dist = ho.hamming(t.queries, rows)
    assign = None
    if ivf:
        assign = idx.export_assign()
        assert np.array_equal(
            assign, ho.hamming(rows, t.protos).argmin(axis=1))
    adm = admissible(ok, assign, probed if ivf else None)
    got = idx.range_search_binary(t.queries, radius, nprobe=3)
    check(got, dist, row_ids, adm, radius, "after upsert")
    assert np.isin(up_ids, got[2]).any()  # upserted rows are among the hits
    idx.close()


def test_list_mask():
    t = dataset(256)
    idx = make_index(dg.BINARY_IVF_FLAT, t)
    mask = np.ones(NLIST, np.uint8)
    mask[[2, 5, 8]] = 0
    idx.set_list_mask(mask)
    unmasked = mask[t.assign].astype(bool)
    radius = partial_radius(256)
    for nprobe in (3, NLIST):
        adm = admissible(unmasked, t.assign,
                         ho.probed_lists(t.coarse, nprobe))
        got = idx.range_search_binary(t.queries, radius, nprobe=nprobe)
        check(got, t.dist, t.ids, adm, radius, f"mask nprobe={nprobe}")
    idx.set_list_mask(None)
    adm = admissible(np.ones(N, bool), t.assign,
                     ho.probed_lists(t.coarse, NLIST))
    got = idx.range_search_binary(t.queries, radius, nprobe=NLIST)
    check(got, t.dist, t.ids, adm, radius, "mask cleared")
    idx.close()


# ---------------- determinism ----------------
@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_two_calls_are_byte_identical(kind):
    t = dataset(256)
    idx = make_index(kind, t)
    a = idx.range_search_binary(t.queries, 128, nprobe=3)
    b = idx.range_search_binary(t.queries, 128, nprobe=3)
    assert a[0][-1] > 100000  # cross-list hits: many appends race per query
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    idx.close()


# ---------------- statuses ----------------
def test_error_statuses():
    import ctypes as C
    t = dataset(40)
    b = make_index(dg.BINARY_FLAT, t)
    f = dg.Index(dg.FLAT, dg.L2, 32)
    lib = dg.lib()
    lims = np.zeros(3, np.int64)
    out_ids = C.POINTER(C.c_int64)()
    out_dists = C.POINTER(C.c_float)()
    st = lib.dg_range_search_binary(f.h, 2, np.zeros((2, 4), np.uint8), 3, 0,
                                    None, lims, C.byref(out_ids),
                                    C.byref(out_dists))
    assert st == DG_EINVAL and "float" in dg.last_error()
    # both out pointers may be handed to dg_free after a failed call
    lib.dg_free(C.cast(out_ids, C.c_void_p))
    lib.dg_free(C.cast(out_dists, C.c_void_p))
    with pytest.raises(dg.DgError) as e:
        f.range_search_binary(np.zeros((2, 4), np.uint8), 3)
    assert e.value.status == DG_EINVAL
    with pytest.raises(dg.DgError) as e:
        b.range_search(np.zeros((1, 40), np.float32), 3.0)
    assert e.value.status == DG_ENOT_SUPPORT
    assert "dg_range_search_binary" in str(e.value)
    b.close()
    f.close()
