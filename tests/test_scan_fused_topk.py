"""Fused per-wave top-k in the IVF-Flat scan (marked gpu).

The scan keeps each wave's k smallest candidates instead of storing every
candidate; keys and the packed-u64 order are unchanged, so every search must
be BIT-identical to the store-all path (DG_SCAN_FUSED=0, read per call).
Each case runs both paths on one index in one process and also checks, via
dg_last_scan_fused, that the path it meant to exercise is the one that ran.

Shapes are chosen at the edges of the kernel's geometry: a wave owns 256
rows, a block one 1024-row chunk, a query tile 16 queries (8 for the
half-tile instantiation).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"),
                os.path.join(REPO, "dingo-store_amd")]

import pyoracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")

KFUSE_MAX = 64  # dg_index::kScanFuseMaxK
D = 32
# partial last wave, whole idle waves, chunk boundary, a third chunk of one
# row, lengths that are no multiple of 4
LENS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 2049]
NLIST = len(LENS)
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
N = int(OFF[-1])
# queries per list at nprobe=1: half tile, full tile, second and third tile
QPL = [1, 8, 9, 16, 17, 33, 1, 8, 17]


def ids_match_with_tie_slack(gd, gi, od, oi, tol=1e-3):
    """Rows may disagree only where distances tie within tol (same rule as
    test_gpu_parity.py)."""
    exact = (gi == oi)
    if exact.all():
        return 1.0
    bad = 0
    for r in range(gi.shape[0]):
        if exact[r].all():
            continue
        if not np.allclose(np.sort(gd[r]), np.sort(od[r]), rtol=tol,
                           atol=tol):
            bad += 1
            continue
        for c in np.nonzero(~exact[r])[0]:
            if abs(gd[r, c] - od[r, c]) > tol * max(1.0, abs(od[r, c])):
                bad += 1
                break
    return 1.0 - bad / gi.shape[0]


def _centroids():
    c = np.zeros((NLIST, D), np.float32)
    c[np.arange(NLIST), np.arange(NLIST)] = 10.0
    return c


def _near(cents, lists, rng, sigma=0.1):
    x = cents[lists] + rng.normal(0, sigma, (len(lists), D))
    return np.ascontiguousarray(x, np.float32)


@pytest.fixture(scope="module")
def data():
    """Rows grouped list by list (row id == position, so an id range is a
    row range of one list) around well-separated centroids, so list lengths
    are exactly LENS under every metric."""
    rng = np.random.default_rng(20261020)
    cents = _centroids()
    base = _near(cents, np.repeat(np.arange(NLIST), LENS), rng)
    q_one = _near(cents, np.repeat(np.arange(NLIST), QPL), rng)
    q_all = _near(cents, rng.integers(0, NLIST, 33), rng)
    return cents, base, q_one, q_all


def _index(metric, cents, base):
    idx = dg.Index(dg.IVF_FLAT, metric, D, nlist=NLIST)
    idx.set_centroids(cents)
    idx.add(np.arange(len(base), dtype=np.int64), base)
    return idx


@pytest.fixture(scope="module")
def l2_index(data):
    cents, base, _, _ = data
    idx = _index(dg.L2, cents, base)
    yield idx
    idx.close()


def _search(idx, fused, q, k, nprobe, filt=None, calls=1):
    """calls searches under one DG_SCAN_FUSED setting; returns the results
    and which path the library reports."""
    old = os.environ.get("DG_SCAN_FUSED")
    try:
        if fused:
            os.environ.pop("DG_SCAN_FUSED", None)
        else:
            os.environ["DG_SCAN_FUSED"] = "0"
        out = [idx.search(q, k, nprobe=nprobe, filt=filt)
               for _ in range(calls)]
        return out, idx.last_scan_fused()
    finally:
        if old is None:
            os.environ.pop("DG_SCAN_FUSED", None)
        else:
            os.environ["DG_SCAN_FUSED"] = old


def both_paths(idx, q, k, nprobe, filt=None, calls=1, expect_fused=True):
    """Fused and store-all results must be bit-identical; returns them."""
    f, was_fused = _search(idx, True, q, k, nprobe, filt, calls)
    u, was_fused_off = _search(idx, False, q, k, nprobe, filt, calls)
    assert was_fused == expect_fused
    assert not was_fused_off
    for d_, i_ in f + u[1:]:
        assert np.array_equal(i_, u[0][1])
        assert np.array_equal(d_.view(np.uint32), u[0][0].view(np.uint32))
    return u[0]


@pytest.mark.parametrize("metric", [dg.L2, dg.IP, dg.COSINE])
def test_wave_chunk_and_tile_edges(data, metric):
    """nprobe=1: every list length in LENS is scanned by QPL queries; lists
    shorter than k give -1/0.0 padding out of never-written slots."""
    cents, base, q_one, _ = data
    idx = _index(metric, cents, base)
    try:
        gd, gi = both_paths(idx, q_one, 10, 1)
    finally:
        idx.close()
    lists = np.repeat(np.arange(NLIST), QPL)
    for r, l in enumerate(lists):
        got = gi[r][gi[r] >= 0]
        assert len(got) == min(10, LENS[l])
        assert ((got >= OFF[l]) & (got < OFF[l + 1])).all()
        assert (gd[r][gi[r] < 0] == 0.0).all()
    if metric == dg.L2:
        assign = orc.ivf_assign(orc.L2, base, cents)
        assert np.array_equal(np.bincount(assign, minlength=NLIST), LENS)
        off, gv, gids = orc.ivf_build(base, None, NLIST, assign)
        od, oi = orc.ivf_search(orc.L2, cents, off, gv, gids, q_one, 10, 1)
        assert ids_match_with_tie_slack(gd, gi, od, oi) >= 0.99


@pytest.mark.parametrize("k", [1, 10, KFUSE_MAX, KFUSE_MAX + 1])
def test_k_values(data, l2_index, k):
    """k up to KFUSE_MAX is fused, KFUSE_MAX + 1 falls back; both match."""
    _, _, q_one, _ = data
    both_paths(l2_index, q_one, k, 3, expect_fused=k <= KFUSE_MAX)


def test_full_sweep(data, l2_index):
    """nprobe == nlist: 33 queries on every list (three query tiles)."""
    _, _, _, q_all = data
    gd, gi = both_paths(l2_index, q_all, 10, NLIST)
    assert (gi >= 0).all()


@pytest.mark.parametrize("nq", [1, 3])
def test_small_batch_graph_replay(data, l2_index, nq):
    """nq <= 4 without a filter: the second call replays a captured graph,
    which must hold the path that was current when it was captured."""
    _, _, _, q_all = data
    both_paths(l2_index, q_all[:nq], 10, 4, calls=2)


def test_exact_duplicates(data):
    """Equal keys resolve to the smaller CSR row on both paths: 40 copies of
    one vector spread over lanes and waves of a 300-row list."""
    cents, _, _, _ = data
    rng = np.random.default_rng(7)
    lists = np.repeat(np.arange(NLIST), [300] + [5] * (NLIST - 1))
    base = _near(cents, lists, rng)
    dup = np.sort(rng.choice(300, 40, replace=False))
    base[dup] = base[dup[0]]
    q = np.repeat(base[dup[:1]], 9, axis=0)
    idx = _index(dg.L2, cents, base)
    try:
        gd, gi = both_paths(idx, q, 10, 1)
    finally:
        idx.close()
    assert np.isin(gi, dup).all()
    assert (gd == gd[0, 0]).all()
    assert all(len(set(r)) == 10 for r in gi.tolist())


def test_range_filter(data, l2_index):
    """A filter that leaves 40 rows of one chunk and none of any other
    probed list; then one that leaves nothing of the only probed list."""
    _, _, q_one, q_all = data
    lo = int(OFF[8]) + 1000
    f = dg.make_filter(kind=1, min_id=lo, max_id=lo + 40)
    gd, gi = both_paths(l2_index, q_all, 10, NLIST, filt=f)
    assert ((gi >= lo) & (gi < lo + 40)).all()
    gd, gi = both_paths(l2_index, q_one[:10], 10, 1, filt=f)
    assert (gi == -1).all() and (gd == 0.0).all()


def test_list_mask(data, l2_index):
    _, _, q_one, q_all = data
    mask = (np.arange(NLIST) % 2).astype(np.uint8)
    l2_index.set_list_mask(mask)
    try:
        gd, gi = both_paths(l2_index, q_all, 10, NLIST)
        both_paths(l2_index, q_one, 10, 3)
    finally:
        l2_index.set_list_mask(None)
    owner = np.searchsorted(OFF, gi[gi >= 0], side="right") - 1
    assert (mask[owner] == 1).all()


def test_range_search_after_fused(data, l2_index):
    """Range search consumes all candidates: it keeps the store-all path,
    also on an index whose workspaces were last used by fused searches."""
    cents, base, _, q_all = data
    (gd, _), = _search(l2_index, True, q_all, 10, NLIST)[0]
    assert l2_index.last_scan_fused()
    radius = float(np.median(gd[:, 5]))
    lims, dists, ids = l2_index.range_search(q_all, radius)
    assert not l2_index.last_scan_fused()
    assign = orc.ivf_assign(orc.L2, base, cents)
    off, gv, gids = orc.ivf_build(base, None, NLIST, assign)
    ol, od, oi = orc.ivf_range_search(orc.L2, cents, off, gv, gids, q_all,
                                      radius, NLIST)
    assert np.array_equal(lims, ol) and lims[-1] > 0
    # each query's hits come best-first; near-equal distances may swap places
    # between the two engines, so compare members and sorted distances
    for a, b in zip(lims[:-1], lims[1:]):
        assert np.array_equal(np.sort(ids[a:b]), np.sort(oi[a:b]))
        assert np.allclose(np.sort(dists[a:b]), np.sort(od[a:b]), rtol=1e-3,
                           atol=1e-3)
