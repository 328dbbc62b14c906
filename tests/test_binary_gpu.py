"""Binary (Hamming) Flat and IVF-Flat indexes on the GPU (marked gpu).

Reference: the numpy Hamming oracle in hamming_oracle.py.  Hamming ties are
the norm, so rows are accepted by the exact rule of hamming_oracle.check_row
(no tolerance, no skipped rows), never by comparing ids positionally.  IVF
list membership is taken from export_assign() — after asserting that every
assignment is the minimum-Hamming centroid with ties toward the smaller
list — and the probed lists are recomputed by (distance, list id).

Shapes sit at the edges of the kernels' geometry: a scan thread owns 4 rows,
a block one 1024-row chunk, a query tile 8 queries; rows are padded to
32-bit words.
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

DG_EINVAL, DG_ENOT_SUPPORT, DG_EID_DUPLICATED, DG_ENOT_FOUND = 1, 3, 8, 9
# one byte, word + tail, whole words, 31 1/4 words with an odd tail
DIMS = [8, 40, 256, 1000]
# partial thread quad, idle waves, chunk boundary, a third chunk of one row
LENS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 2049]
NLIST = len(LENS)
N = sum(LENS)
# queries per list: below / at / above one and two 8-query tiles
QPL = [1, 8, 9, 16, 17, 33, 1, 8, 17]
NPROBES = [1, 3, NLIST]
KS = [1, 10, 100]  # 100 exceeds several lists: padding


class Data:
    pass


@functools.lru_cache(maxsize=None)
def dataset(d):
    """Prototype codes as injected centroids; base rows and queries are a
    prototype with 5 % of the bits flipped.  Computed once per d and never
    modified (tests that mutate work on copies)."""
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


def make_index(kind, t, add=True):
    idx = dg.Index(kind, dg.HAMMING, t.d, nlist=NLIST)
    if kind == dg.BINARY_IVF_FLAT:
        idx.set_centroids(t.protos)
    if add:
        idx.add(t.ids, t.base)
    return idx


def verify(dist, ids, oracle_dist, row_ids, row_ok, assign=None, probed=None,
           where=""):
    """check_row for every query; admissible = row_ok and, for IVF, in a
    probed list."""
    for q in range(dist.shape[0]):
        ok = row_ok
        if assign is not None:
            lut = np.zeros(NLIST + 1, bool)
            lut[probed[q]] = True
            ok = ok & lut[assign]
        ho.check_row(dist[q], ids[q], row_ids[ok], oracle_dist[q][ok],
                     where=f"{where} q={q}")


ALL = np.ones(N, bool)


# ---------------- geometry sweep ----------------
@pytest.mark.parametrize("d", DIMS)
def test_ivf_geometry_sweep(d):
    t = dataset(d)
    idx = make_index(dg.BINARY_IVF_FLAT, t)
    assign = idx.export_assign()
    # minimum-Hamming centroid, ties toward the smaller list
    assert np.array_equal(assign, t.assign)
    for nprobe in NPROBES:
        probed = ho.probed_lists(t.coarse, nprobe)
        for k in KS:
            gd, gi = idx.search(t.queries, k, nprobe=nprobe)
            verify(gd, gi, t.dist, t.ids, ALL, assign, probed,
                   where=f"d={d} nprobe={nprobe} k={k}")
    st = idx.stats()
    assert st["d"] == d and st["kind"] == dg.BINARY_IVF_FLAT
    assert st["ntotal"] == N and st["nlist"] == NLIST
    # last search probed every list: algorithmic bytes = probed rows x d/8
    assert st["last_scan_bytes_algorithmic"] == N * (d // 8)
    idx.close()


@pytest.mark.parametrize("d", DIMS)
def test_flat_geometry_sweep(d):
    t = dataset(d)
    idx = make_index(dg.BINARY_FLAT, t)
    for k in KS:
        gd, gi = idx.search(t.queries, k)
        verify(gd, gi, t.dist, t.ids, ALL, where=f"flat d={d} k={k}")
    st = idx.stats()
    assert st["d"] == d and st["kind"] == dg.BINARY_FLAT
    assert st["last_scan_bytes_algorithmic"] == N * (d // 8)
    assert st["device_bytes"] >= N * (d // 8)
    idx.close()


@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_fewer_rows_than_k(kind):
    t = dataset(40)
    idx = dg.Index(kind, dg.HAMMING, 40, nlist=NLIST)
    if kind == dg.BINARY_IVF_FLAT:
        idx.set_centroids(t.protos)
    idx.add(t.ids[:5], t.base[:5])
    gd, gi = idx.search(t.queries[:7], 10, nprobe=NLIST)
    verify(gd, gi, t.dist[:7, :5], t.ids[:5], np.ones(5, bool))
    assert (gi[:, 5:] == -1).all() and (gi[:, :5] >= 0).all()
    idx.close()


def test_k_zero_is_noop():
    t = dataset(40)
    idx = make_index(dg.BINARY_FLAT, t)
    dist = np.full((2, 1), 5.0, np.float32)
    ids = np.full((2, 1), 5, np.int64)
    st = dg.lib().dg_search_binary(idx.h, 2, t.queries[:2].copy(), 0, 0,
                                   None, dist, ids)
    assert st == 0 and (dist == 5.0).all() and (ids == 5).all()
    idx.close()


# ---------------- determinism / device-pointer form ----------------
@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_deterministic_and_device_form(kind):
    import torch
    t = dataset(256)
    idx = make_index(kind, t)
    k, nprobe = 10, 3
    d1, i1 = idx.search(t.queries, k, nprobe=nprobe)
    d2, i2 = idx.search(t.queries, k, nprobe=nprobe)
    assert d1.tobytes() == d2.tobytes() and i1.tobytes() == i2.tobytes()
    nq = t.queries.shape[0]
    tq = torch.from_numpy(t.queries.copy()).cuda()
    td = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ti = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    idx.search_device(tq.data_ptr(), nq, k, nprobe, td.data_ptr(),
                      ti.data_ptr())
    idx.sync()
    assert td.cpu().numpy().tobytes() == d1.tobytes()
    assert ti.cpu().numpy().tobytes() == i1.tobytes()
    idx.close()


# ---------------- filters ----------------
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
    for name, filt, ok in _filters(t):
        assert 0 < ok.sum() < N, name
        gd, gi = idx.search(t.queries, 10, nprobe=3, filt=filt)
        verify(gd, gi, t.dist, t.ids, ok, t.assign if ivf else None,
               probed if ivf else None, where=name)
    idx.close()


# ---------------- mutation ----------------
@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_remove_upsert_and_id_errors(kind):
    t = dataset(256)
    idx = make_index(kind, t)
    ivf = kind == dg.BINARY_IVF_FLAT
    rng = np.random.default_rng(5)
    probed = ho.probed_lists(t.coarse, 3)

    gone = rng.choice(N, N // 10, replace=False)
    idx.remove(t.ids[gone])
    alive = ALL.copy()
    alive[gone] = False
    assert idx.stats()["ntotal"] == N - len(gone)
    gd, gi = idx.search(t.queries, 10, nprobe=3)
    verify(gd, gi, t.dist, t.ids, alive, t.assign if ivf else None,
           probed if ivf else None, where="after remove")

    # upsert: live rows with changed bits, removed rows coming back, new ids
    live_rows = np.nonzero(alive)[0]
    up_rows = np.concatenate([rng.choice(live_rows, 40, replace=False),
                              gone[:10]])
    up_ids = np.concatenate([t.ids[up_rows], [900001, 900002, 900003]])
    up_codes = ho.flip_bits(
        t.base[np.concatenate([up_rows, [0, 300, 5000]])], 0.2, rng)
    idx.upsert(up_ids, up_codes)
    rows = np.concatenate([t.base, up_codes])
    row_ids = np.concatenate([t.ids, up_ids])
    ok = np.concatenate([alive & ~np.isin(t.ids, up_ids),
                         np.ones(len(up_ids), bool)])
    assert idx.stats()["ntotal"] == ok.sum()
    dist = ho.hamming(t.queries, rows)
    assign = None
    if ivf:
        assign = idx.export_assign()
        assert np.array_equal(
            assign, ho.hamming(rows, t.protos).argmin(axis=1))
    gd, gi = idx.search(t.queries, 10, nprobe=3)
    verify(gd, gi, dist, row_ids, ok, assign, probed if ivf else None,
           where="after upsert")

    # duplicate ids in one add; remove of a missing id removes nothing
    before = idx.stats()["ntotal"]
    with pytest.raises(dg.DgError) as e:
        idx.add(np.array([800001, 800001], np.int64), t.base[:2])
    assert e.value.status == DG_EID_DUPLICATED
    with pytest.raises(dg.DgError) as e:
        idx.remove(np.array([int(row_ids[ok][0]), 123456789], np.int64))
    assert e.value.status == DG_ENOT_FOUND
    assert idx.stats()["ntotal"] == before
    gd2, gi2 = idx.search(t.queries, 10, nprobe=3)
    assert gd2.tobytes() == gd.tobytes() and gi2.tobytes() == gi.tobytes()
    idx.close()


def test_list_mask():
    t = dataset(256)
    idx = make_index(dg.BINARY_IVF_FLAT, t)
    mask = np.ones(NLIST, np.uint8)
    mask[[2, 5, 8]] = 0
    idx.set_list_mask(mask)
    unmasked = mask[t.assign].astype(bool)
    for nprobe in (3, NLIST):
        probed = ho.probed_lists(t.coarse, nprobe)
        gd, gi = idx.search(t.queries, 10, nprobe=nprobe)
        verify(gd, gi, t.dist, t.ids, unmasked, t.assign, probed,
               where=f"mask nprobe={nprobe}")
    idx.set_list_mask(None)
    gd, gi = idx.search(t.queries, 10, nprobe=NLIST)
    verify(gd, gi, t.dist, t.ids, ALL, t.assign,
           ho.probed_lists(t.coarse, NLIST), where="mask cleared")
    idx.close()


# ---------------- contract edges ----------------
def test_untrained_ivf_returns_blank():
    t = dataset(40)
    idx = dg.Index(dg.BINARY_IVF_FLAT, dg.HAMMING, 40, nlist=NLIST)
    assert idx.stats()["is_trained"] == 0
    gd, gi = idx.search(t.queries[:4], 5, nprobe=3)
    assert (gi == -1).all()
    with pytest.raises(dg.DgError):  # add needs centroids
        idx.add(t.ids[:4], t.base[:4])
    idx.close()


def test_entry_point_mismatch_is_einval():
    t = dataset(256)
    lib = dg.lib()
    b = make_index(dg.BINARY_FLAT, t)
    f = dg.Index(dg.FLAT, dg.L2, 32)
    xf = np.zeros((2, 256), np.float32)
    xb = np.zeros((2, 4), np.uint8)
    ids = np.array([1, 2], np.int64)
    od = np.empty((2, 1), np.float32)
    oi = np.empty((2, 1), np.int64)
    # float entry points on a binary index
    for st in (lib.dg_add(b.h, 2, ids, xf), lib.dg_upsert(b.h, 2, ids, xf),
               lib.dg_train(b.h, 2, xf),
               lib.dg_set_centroids(b.h, 1, xf),
               lib.dg_get_centroids(b.h, xf),
               lib.dg_search(b.h, 2, xf, 1, 0, None, od, oi)):
        assert st == DG_EINVAL
        assert "binary" in dg.last_error()
    # binary entry points on a float index
    for st in (lib.dg_add_binary(f.h, 2, ids, xb),
               lib.dg_upsert_binary(f.h, 2, ids, xb),
               lib.dg_train_binary(f.h, 2, xb),
               lib.dg_set_centroids_binary(f.h, 1, xb),
               lib.dg_get_centroids_binary(f.h, xb),
               lib.dg_search_binary(f.h, 2, xb, 1, 0, None, od, oi)):
        assert st == DG_EINVAL
        assert "float" in dg.last_error()
    assert b.stats()["ntotal"] == N and f.stats()["ntotal"] == 0
    b.close()
    f.close()


@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_unsupported_calls(kind, tmp_path):
    t = dataset(40)
    idx = make_index(kind, t)
    with pytest.raises(dg.DgError) as e:
        idx.range_search(np.zeros((1, 40), np.float32), 3.0)
    assert e.value.status == DG_ENOT_SUPPORT
    for fn in (idx.save, idx.save_faiss):
        with pytest.raises(dg.DgError) as e:
            fn(str(tmp_path / "binary.idx"))
        assert e.value.status == DG_ENOT_SUPPORT
    idx.close()


@pytest.mark.parametrize("kind", [dg.BINARY_FLAT, dg.BINARY_IVF_FLAT])
def test_bad_creates(kind):
    for d, metric in ((12, dg.HAMMING), (64, dg.L2), (64, dg.IP)):
        with pytest.raises(dg.DgError) as e:
            dg.Index(kind, metric, d, nlist=4)
        assert e.value.status == DG_EINVAL


# ---------------- train ----------------
def test_train_quality_and_degrade():
    d, nlist, n = 256, 8, 2000
    rng = np.random.default_rng(20261020)
    protos = rng.integers(0, 256, (nlist, d // 8), dtype=np.uint8)
    x = ho.flip_bits(protos[rng.integers(0, nlist, n)], 0.05, rng)
    idx = dg.Index(dg.BINARY_IVF_FLAT, dg.HAMMING, d, nlist=nlist)
    idx.train(x)
    assert idx.stats()["is_trained"] == 1
    cents = idx.get_centroids()
    assert cents.shape == (nlist, d // 8)
    trained = ho.hamming(x, cents).min(axis=1).mean()
    first_rows = ho.hamming(x, x[:nlist]).min(axis=1).mean()
    print(f"mean distance to nearest centroid: trained {trained:.2f}, "
          f"first-{nlist}-rows {first_rows:.2f}")
    assert trained <= first_rows
    idx.train(x[:100])  # already trained: OK no-op
    assert np.array_equal(idx.get_centroids(), cents)
    # trained index is searchable and exact against its own structure
    ids = np.arange(n, dtype=np.int64)
    idx.add(ids, x)
    assign = idx.export_assign()
    assert np.array_equal(assign, ho.hamming(x, cents).argmin(axis=1))
    q = x[:33]
    gd, gi = idx.search(q, 10, nprobe=3)
    probed = ho.probed_lists(ho.hamming(q, cents), 3)
    dist = ho.hamming(q, x)
    for r in range(len(q)):
        ok = np.isin(assign, probed[r])
        ho.check_row(gd[r], gi[r], ids[ok], dist[r][ok], where=f"train q={r}")
    idx.close()

    # n < nlist degrades to nlist = 1; searches then equal Flat
    small = dg.Index(dg.BINARY_IVF_FLAT, dg.HAMMING, d, nlist=nlist)
    small.train(x[:5])
    st = small.stats()
    assert st["is_trained"] == 1 and st["nlist"] == 1
    flat = dg.Index(dg.BINARY_FLAT, dg.HAMMING, d)
    small.add(ids[:1500], x[:1500])
    flat.add(ids[:1500], x[:1500])
    d1, i1 = small.search(x[1500:1540], 10, nprobe=4)
    d2, i2 = flat.search(x[1500:1540], 10)
    # same distances; ids by the acceptance rule (the row order inside a
    # list is fixed at finalize and differs between two indexes, so tied
    # ids may legitimately differ)
    assert d1.tobytes() == d2.tobytes()
    oracle = ho.hamming(x[1500:1540], x[:1500])
    verify(d1, i1, oracle, ids[:1500], np.ones(1500, bool), where="degraded")
    verify(d2, i2, oracle, ids[:1500], np.ones(1500, bool), where="flat")
    small.close()
    flat.close()


# ---------------- C++ mirror ----------------
def test_mirror_selftest_binary():
    assert dg.lib().dg_mirror_selftest_binary() == 0
