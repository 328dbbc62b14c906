"""4-bit IVF-PQ (nbits=4): encode pipeline + k_ivfpq4_scan against the float64
ADC reference of pq_reference.py (marked gpu).

Method, bound and checks A-D: pq_reference.py and test_ivfpq_scan.py.  The
bound allows one f16 rounding per S and T entry and 2m + 3 f32 roundings,
which leaves room for the folded table U = S - 2T.  Every case asserts on
the reference alone that max b <= 5 % of the median k-th distance.

Geometry: packed rows of m/2 bytes, 256-row tiles of 1024-row chunks, a
list's probing queries split over 4 waves; m/8 dwords per row.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "dingo-store_amd"), HERE]

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")

from pq_reference import (Case, HALF_MAX, add_all,  # noqa: E402
                          grouped_case)

# one row, under a wave, around the 256-row tile, around the 1024-row chunk,
# a third chunk of one row
LENS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 2049]
# queries per list at nprobe=1 over 4 waves: one wave busy, all four, a
# second round of one, two full rounds, a third round
QPL = [1, 4, 5, 8, 9, 1, 4, 5, 9]

_CACHE = {}


@pytest.fixture(scope="module")
def lens_index():
    """The LENS geometry per metric, built on first use and never mutated."""
    def get(metric):
        if metric not in _CACHE:
            case, lists, codes, x32 = grouped_case(metric, 32, 8, LENS,
                                                   2000 + metric)
            idx = case.new_index()
            add_all(case, idx, lists, codes, x32)
            q_one = case.queries(np.repeat(np.arange(len(LENS)), QPL))
            q_all = case.queries(case.rng.integers(0, len(LENS), 33))
            _CACHE[metric] = (case, idx, q_one, q_all)
        return _CACHE[metric]
    yield get
    for _, idx, _, _ in _CACHE.values():
        idx.close()
    _CACHE.clear()


@pytest.mark.parametrize("metric", [dg.L2, dg.IP, dg.COSINE])
def test_list_length_edges(lens_index, metric):
    """nprobe=1: every list length in LENS is scanned by QPL queries (1, 4,
    5, 8 and 9 per list: the rounds of the four waves)."""
    case, idx, q_one, _ = lens_index(metric)
    gd, gi = idx.search(q_one, 10, nprobe=1)
    case.check(q_one, 10, 1, gd, gi)
    for r, l in enumerate(np.repeat(np.arange(len(LENS)), QPL)):
        assert (gi[r] >= 0).sum() == min(10, LENS[l])


@pytest.mark.parametrize("metric", [dg.L2, dg.IP, dg.COSINE])
def test_all_lists_33_queries(lens_index, metric):
    """nprobe == nlist: 33 queries on every list, nine rounds of the four
    waves, candidates of nine lists merged per query."""
    case, idx, _, q_all = lens_index(metric)
    gd, gi = idx.search(q_all, 10, nprobe=len(LENS))
    case.check(q_all, 10, len(LENS), gd, gi)


@pytest.mark.parametrize("k", [1, 10, 100])
def test_k_values(lens_index, k):
    """k below, at and above the rows of the probed list (1, 3 and 255-row
    lists at k=100 leave -1 / 0.0 slots)."""
    case, idx, q_one, _ = lens_index(dg.L2)
    gd, gi = idx.search(q_one, k, nprobe=1)
    case.check(q_one, k, 1, gd, gi)


@pytest.mark.parametrize("metric", [dg.L2, dg.IP])
@pytest.mark.parametrize("d,m", [(32, 16), (48, 24), (16, 8), (16, 16)])
def test_subspace_counts(metric, d, m):
    """m=16: two dwords per packed row; m=24: three (not a power of two, odd
    LDS stride without padding); m=8 at d=16: one dword, dsub=2; m=16 at
    d=16: dsub=1."""
    lens = [300, 257, 40]
    case, lists, codes, x32 = grouped_case(metric, d, m, lens, 77 + m + d)
    idx = case.new_index()
    try:
        add_all(case, idx, lists, codes, x32)
        q = case.queries(np.repeat(np.arange(3), [4, 3, 2]))
        for nprobe in (1, 3):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


def test_insertion_order_and_ids():
    """Rows arrive shuffled across lists in two add calls with ids that are
    not positions: nibble order in the encoder, the packed gather's
    permutation and the id lookup."""
    lens = [300, 257, 1025]
    case, lists, codes, x32 = grouped_case(dg.L2, 32, 8, lens, 31)
    perm = case.rng.permutation(len(lists))
    lists, codes, x32 = lists[perm], codes[perm], x32[perm]
    ids = 7 * np.arange(len(lists), dtype=np.int64) + 3
    cut = 700
    idx = case.new_index()
    try:
        add_all(case, idx, lists[:cut], codes[:cut], x32[:cut], ids[:cut])
        add_all(case, idx, lists[cut:], codes[cut:],
                np.ascontiguousarray(x32[cut:]), ids[cut:])
        q = case.queries(np.repeat(np.arange(3), 3))
        for nprobe in (1, 3):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


def test_filters_mask_and_mutation():
    """Filters, a list mask, tombstones and upserts on the 4-bit scan."""
    case, lists, codes, x32 = grouped_case(dg.L2, 32, 8, LENS, 47)
    off = np.concatenate([[0], np.cumsum(LENS)])
    nl = len(LENS)
    idx = case.new_index()
    try:
        add_all(case, idx, lists, codes, x32)
        q_one = case.queries(np.repeat(np.arange(nl), 2))
        q_all = case.queries(case.rng.integers(0, nl, 9))

        # 40 rows of the second tile of the 2049-row list, nothing else
        lo = int(off[8]) + 300
        f = dg.make_filter(kind=1, min_id=lo, max_id=lo + 40)
        in_range = lambda ids: (ids >= lo) & (ids < lo + 40)  # noqa: E731
        gd, gi = idx.search(q_all, 10, nprobe=nl, filt=f)
        case.check(q_all, 10, nl, gd, gi, keep=in_range)
        assert ((gi >= lo) & (gi < lo + 40)).all()
        # the same filter leaves nothing of the lists probed at nprobe=1
        gd, gi = idx.search(q_one[:16], 10, nprobe=1, filt=f)
        case.check(q_one[:16], 10, 1, gd, gi, keep=in_range)
        assert (gi == -1).all() and (gd == 0.0).all()

        # sorted ids, plain and negated
        pick = np.sort(case.rng.choice(len(lists), 1500, replace=False))
        for neg in (False, True):
            f = dg.make_filter(kind=2, ids=pick, negate=neg)
            keep = (lambda ids, neg=neg: np.isin(ids, pick) != neg)
            gd, gi = idx.search(q_one, 10, nprobe=1, filt=f)
            case.check(q_one, 10, 1, gd, gi, keep=keep)

        # list mask: probes of masked lists are dropped
        mask = (np.arange(nl) % 2).astype(np.uint8)
        idx.set_list_mask(mask)
        try:
            gd, gi = idx.search(q_all, 10, nprobe=nl)
            case.check(q_all, 10, nl, gd, gi, mask=mask)
            gd, gi = idx.search(q_one, 10, nprobe=1)
            case.check(q_one, 10, 1, gd, gi, mask=mask)
        finally:
            idx.set_list_mask(None)

        # tombstones across the first tile boundary of the 1025-row list and
        # across its chunk boundary
        gone = np.concatenate([np.arange(off[7] + 250, off[7] + 262),
                               np.arange(off[7] + 1020, off[7] + 1025)])
        idx.remove(gone)
        case.forget(gone)
        gd, gi = idx.search(q_one, 10, nprobe=1)
        case.check(q_one, 10, 1, gd, gi)
        assert not np.isin(gi, gone).any()

        # upsert: some removed ids come back, some live ids move list
        up_ids = np.concatenate([gone[:6], np.arange(off[4], off[4] + 5),
                                 np.arange(off[8] + 255, off[8] + 258)])
        up_lists = case.rng.integers(0, nl, len(up_ids))
        up_codes, up_x = case.make_rows(up_lists)
        idx.upsert(up_ids, up_x)
        case.record(up_ids, up_lists, up_codes)
        for q, nprobe in ((q_one, 1), (q_all, nl)):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


def test_range_search(lens_index):
    """L2 range search: the returned set is the reference set, up to rows
    whose reference distance is within b of the radius."""
    case, idx, _, q_all = lens_index(dg.L2)
    q = q_all[:9]
    # a radius that takes a part of the query's own list: the median of the
    # reference distances to the rows of the nearest list
    Q = case._unit(q)
    near = [np.sort(case.reference(x)[2][case.lists ==
                                         case.coarse_keys(x).argmin()])
            for x in Q]
    radius = float(np.median([np.median(n) for n in near]))
    lims, gd, gi = idx.range_search(q, radius)
    sizes = case.range_check(q, radius, lims, gd, gi)
    assert max(sizes) > 100 and min(sizes) < max(sizes)  # not vacuous


def test_m_limit():
    """m above the LDS limit is refused at create with the limit in the
    message; the largest accepted m (dsub=1, two short lists) passes A-D."""
    m = dg.ivfpq_max_m_nbits(0, 4)
    assert dg.ivfpq_max_m_nbits(0, 8) == dg.ivfpq_max_m()
    assert m > dg.ivfpq_max_m() and m % 8 == 0
    assert dg.ivfpq_max_m_nbits(0, 5) == 0
    with pytest.raises(dg.DgError) as e:
        dg.Index(dg.IVF_PQ, dg.L2, m + 8, nlist=2, m=m + 8, nbits=4)
    assert e.value.status == 3  # DG_ENOT_SUPPORT
    assert str(m) in str(e.value)
    case, lists, codes, x32 = grouped_case(dg.L2, m, m, [257, 43], 9)
    idx = case.new_index()
    try:
        add_all(case, idx, lists, codes, x32)
        q = case.queries(np.array([0, 0, 1, 1, 0]))
        for nprobe in (1, 2):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


@pytest.mark.parametrize("nbits,m", [(3, 8), (5, 8), (12, 8), (4, 12)])
def test_unsupported_geometry_is_refused(nbits, m):
    with pytest.raises(dg.DgError) as e:
        dg.Index(dg.IVF_PQ, dg.L2, 48, nlist=4, m=m, nbits=nbits)
    assert e.value.status == 3  # DG_ENOT_SUPPORT
    if nbits != 4:
        assert "{4, 8}" in str(e.value)


@pytest.mark.parametrize("nbits", [8, 0])
def test_default_width_still_creates(nbits):
    idx = dg.Index(dg.IVF_PQ, dg.L2, 48, nlist=4, m=12, nbits=nbits)
    try:
        assert idx.nbits == 8
        # 256-entry codebooks are what it takes
        case = Case(dg.L2, 48, 12, 4, 5, nbits=8)
        idx.set_centroids(case.cents32)
        idx.set_codebooks(case.cb32)
        assert idx.get_codebooks().shape == (12, 256, 4)
    finally:
        idx.close()


def test_codebooks_round_trip_and_width_mismatch():
    case = Case(dg.L2, 32, 8, 3, 5)
    idx = case.new_index()
    try:
        got = idx.get_codebooks()
        assert got.shape == (8, 16, 4)
        assert np.array_equal(got, case.cb32)
        with pytest.raises(dg.DgError):  # 256-entry books on a 4-bit index
            idx.set_codebooks(np.zeros((8, 256, 4), np.float32))
    finally:
        idx.close()


def _scale_for_max_s(target):
    probe = Case(dg.L2, 32, 8, 3, 63)
    return float(np.sqrt(target / probe.S.max()))


def test_table_overflow_is_refused():
    """max S above the f16 range: set_codebooks fails loudly."""
    case = Case(dg.L2, 32, 8, 3, 63, scale=_scale_for_max_s(7.0e4))
    assert case.S.max() > HALF_MAX
    idx = dg.Index(dg.IVF_PQ, dg.L2, 32, nlist=3, m=8, nbits=4)
    try:
        idx.set_centroids(case.cents32)
        with pytest.raises(dg.DgError) as e:
            idx.set_codebooks(case.cb32)
        assert e.value.status == 3  # DG_ENOT_SUPPORT
        assert "65504" in str(e.value)
    finally:
        idx.close()
