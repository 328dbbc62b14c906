"""float64 reference model of an IVF-Flat search, the shape tables and the
input generators of test_ivf_exact.py (GPU) and test_ivf_reference_cpu.py.

The distances, the bound b, the acceptance rules A-D, the range rules, the
strength asserts and the filter model are those of flat_reference.py, used
unchanged: the scan computes key = vnorm - 2 acc with acc an f32 sum of d
products and the emit adds the query norm, which is the structure that bound
was derived for (any summation order; the internal padding adds exact
zeros).  What this module adds is WHICH rows a query may return:

  1. Assignment.  The index's own assignment (export_assign) is read and
     verified (verify_assign): for every row the centroid score of the
     assigned list is within b(row, assigned) + b(row, best) of the best
     float64 score.  Scores, smaller is better: L2 ||c||^2 - 2 x.c (the model
     carries the per-row constant ||x||^2 along, which moves no gap); IP and
     COSINE -x.c over the rows as the index stores them.  For COSINE dg_add
     normalises the rows (k_normalize_rows, before assign_rows) and
     search_core the queries, while dg_set_centroids uploads the centroids
     as given and never normalises them, so the score is -xh.c with xh =
     x / ||x|| and c raw; its bound is (d + 9) u sum|xh_i c_i|, the cosine
     bound of flat_reference with only one side normalised.  The verified
     assignment then defines the lists: a near-tie row may sit in either
     list, a row further than the bound from its best list is a failure of
     k_argmin_rows or the assign GEMM.
  2. Probe set.  Per query the nprobe best lists by the float64 score
     (probe_sets).  The generators produce inputs for which the set is
     unambiguous: the gap between the nprobe-th and the next score exceeds
     the sum of their two bounds for every query (the CPU file asserts zero
     ambiguous queries for every table below).  No list mask is used.
  3. Eligible rows of a query: rows of its probed lists that are not removed
     and pass the filter, a bool [nq, n] handed to check_topk / check_range.

Kernel geometry the shapes rest on (k_ivf_scan_pipe, dg_scan_rows_body,
ivf_scan_col / ivf_scan_topk, search_core):
  - a block scans one chunk of 1024 rows of one list; a wave 256 rows (64
    lanes x 4 rows); chunks are stored dim-major, padded to 4 rows;
  - query tile QTM = 16 for dp <= 2304, 8 for dp <= 4608, 4 above, with
    dp = ceil(d / 4) * 4; only QTM = 16 has the half-tile body, taken when a
    tile holds qt <= 8 queries;
  - the column pipeline has a period of 16 dims; its tail is dp - base in
    {4, 8, 12, 16}; when dp <= 16 only the prologue (which always issues 16
    columns, reading ahead of dp into the slack finalize_csr reserves) and
    the tail run;
  - a search is fused (per-wave top-k inside the scan) iff k <= 64 and
    nprobe * cpl_max * 4 * k <= the sum of the nprobe longest lists and
    DG_SCAN_FUSED is not 0 and it is not a range search; otherwise the scan
    stores every candidate;
  - within a list the CSR order is handed out by an atomic cursor
    (k_scatter_perm), so which rows share a wave or a chunk cannot be fixed
    from outside; the list LENGTHS fix how many waves and chunks there are.

Expected QTM of the case B ladder, derived from the dispatch code and not
observed: d = 2304 -> 16, 2305 (dp 2308) -> 8, 4608 -> 8, 4609 (dp 4612)
-> 4, 8189 (dp 8192) -> 4, 8192 -> 4.

Largest |dist - ref| / b over test_ivf_exact.py on an MI355X (a record, not
a threshold; the threshold is 1):  L2 0.55, IP 0.49,
COSINE 0.23.
"""
import functools
import types

import numpy as np

import flat_reference as fr
from flat_reference import COSINE, IP, L2, U

CHUNK, WAVE_ROWS, KFUSE_MAX, DEFAULT_NPROBE = 1024, 256, 64, 80

# largest observed |dist - ref| / b per metric over the IVF checks
MAX_RATIO = {L2: 0.0, IP: 0.0, COSINE: 0.0}


# --------------------------------------------------------------------------
# geometry
# --------------------------------------------------------------------------
def dp_of(d):
    return (d + 3) // 4 * 4


def qtm_of(d):
    return 16 if dp_of(d) <= 2304 else 8 if dp_of(d) <= 4608 else 4


def tail_of(d):
    """Dims left to the pipeline's epilogue: the loop runs while
    base + 16 < dp."""
    return dp_of(d) - (dp_of(d) - 1) // 16 * 16


def expect_fused(k, nprobe, lens):
    srt = np.sort(np.asarray(lens))[::-1]
    np_ = min(nprobe, len(srt))
    cpl_max = -(-int(srt[0]) // CHUNK)
    return k <= KFUSE_MAX and \
        np_ * cpl_max * (CHUNK // WAVE_ROWS) * k <= int(srt[:np_].sum())


# --------------------------------------------------------------------------
# the model
# --------------------------------------------------------------------------
def coarse_scores(metric, v32, cents32):
    """(score, b), float64 [n, nlist], smaller is better, of rows or queries
    against the centroids."""
    if metric != COSINE:
        ref, b = fr.ref_and_bound(metric, v32, cents32)
        return (ref if metric == L2 else -ref), b
    v = np.asarray(v32, np.float32).astype(np.float64)
    c = np.asarray(cents32, np.float32).astype(np.float64)
    v = v / np.sqrt((v * v).sum(1, keepdims=True))
    return -(v @ c.T), (v.shape[1] + 9) * U * (np.abs(v) @ np.abs(c).T)


def reference_assign(metric, x32, cents32):
    """(assign, unambiguous): the float64 best list of every row, and
    whether each row's runner-up is further than the two bounds."""
    s, b = coarse_scores(metric, x32, cents32)
    order = np.argsort(s, axis=1, kind="stable")
    rows = np.arange(len(s))
    a0, a1 = order[:, 0], order[:, 1]
    clear = s[rows, a1] - s[rows, a0] > b[rows, a0] + b[rows, a1]
    return a0.astype(np.int32), clear


def verify_assign(metric, x32, cents32, assign, where=""):
    """Rule 1 above, every row."""
    s, b = coarse_scores(metric, x32, cents32)
    assign = np.asarray(assign)
    assert assign.shape == (len(s),), (where, assign.shape)
    assert ((assign >= 0) & (assign < s.shape[1])).all(), (where, "list id")
    rows = np.arange(len(s))
    best = np.argmin(s, axis=1)
    bad = s[rows, assign] - s[rows, best] > b[rows, assign] + b[rows, best]
    assert not bad.any(), (where, "row assigned to a list that is not its "
                           "best", np.nonzero(bad)[0][:8], assign[bad][:8],
                           best[bad][:8])


def probe_sets(metric, q32, cents32, nprobe):
    """(probed bool [nq, nlist], ambiguous query indices)."""
    s, b = coarse_scores(metric, q32, cents32)
    nq, nlist = s.shape
    np_ = min(nprobe if nprobe > 0 else DEFAULT_NPROBE, nlist)
    order = np.argsort(s, axis=1, kind="stable")
    probed = np.zeros((nq, nlist), bool)
    np.put_along_axis(probed, order[:, :np_], True, axis=1)
    if np_ == nlist:
        return probed, np.zeros(0, np.int64)
    qi = np.arange(nq)
    last, nxt = order[:, np_ - 1], order[:, np_]
    amb = s[qi, nxt] - s[qi, last] <= b[qi, last] + b[qi, nxt]
    return probed, np.nonzero(amb)[0]


def eligible(probed, assign, admissible):
    """bool [nq, n]: rows of a probed list that are alive and pass."""
    return probed[:, np.asarray(assign)] & np.asarray(admissible)[None, :]


def _recorded(fn, metric, *args, **kw):
    keep = fr.MAX_RATIO[metric]
    try:
        worst = fn(metric, *args, **kw)
    finally:
        fr.MAX_RATIO[metric] = keep  # the Flat table stays the Flat record
    MAX_RATIO[metric] = max(MAX_RATIO[metric], worst)
    return worst


def check_topk(metric, *args, **kw):
    """fr.check_topk; the ratio goes to this module's MAX_RATIO."""
    return _recorded(fr.check_topk, metric, *args, **kw)


def check_range(metric, *args, **kw):
    return _recorded(fr.check_range, metric, *args, **kw)


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def centroids(nlist, d, scale, seed):
    """Equal-norm, well-separated centroids (equal norms make the L2 and the
    IP assignment the same)."""
    c = np.zeros((nlist, d), np.float32)
    if d == 1:
        # one dimension has two directions: under IP a third list can only
        # win exact ties, so list 0 sits at the origin (see make_case)
        assert nlist == 3
        c[:, 0] = [0.0, -scale, scale]
    elif nlist <= 3:
        ang = 2.0 * np.pi * np.arange(nlist) / 3.0
        c[:, 0], c[:, 1] = scale * np.cos(ang), scale * np.sin(ang)
    elif nlist <= d:
        c[np.arange(nlist), np.arange(nlist)] = scale
    else:
        g = np.random.default_rng(seed).standard_normal((nlist, d))
        c[:] = scale * g / np.sqrt((g * g).sum(1, keepdims=True))
    return c


def make_case(seed, lens, d, metric, qlists, scale, sigma, qshift=0.0,
              edge_gain=1.0):
    """Rows list by list around the centroids (row position p has id
    5 p + 11, so an id range is a row range of one list), Gaussian noise of
    sigma per dimension, queries drawn the same way around the centroids
    qlists and moved by the constant qshift.  edge_gain multiplies the noise
    of the last 4 dimensions (see case_b).  At d = 1 under IP / COSINE the
    rows of list 0 are exact zeros: every score of such a row is 0 and the
    tie goes to the smaller list id."""
    rng = np.random.default_rng(seed)
    nlist = len(lens)
    cents = centroids(nlist, d, scale, seed + 1)
    owner = np.repeat(np.arange(nlist), lens).astype(np.int32)
    n = len(owner)
    gain = np.ones(d)
    gain[max(d - 4, 0):] = edge_gain
    x = (cents[owner] + sigma * gain * rng.standard_normal((n, d))).astype(
        np.float32)
    if d == 1 and metric != L2:
        x[owner == 0] = 0.0
    qlists = np.asarray(qlists)
    q = (cents[qlists] +
         sigma * gain * rng.standard_normal((len(qlists), d)) +
         qshift).astype(np.float32)
    if metric == COSINE:  # far from the "already normalised" rule
        assert ((x.astype(np.float64) ** 2).sum(1) > 1.5).all()
        assert ((q.astype(np.float64) ** 2).sum(1) > 1.5).all()
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return types.SimpleNamespace(
        metric=metric, d=d, lens=list(lens), nlist=nlist, n=n, cents=cents,
        x=x, q=q, qlists=qlists, owner=owner, off=off,
        ids=5 * np.arange(n, dtype=np.int64) + 11)


# A. d pipeline at QTM = 16: partial wave, second wave of 4 rows, second
# chunk of 3 rows; 20 queries = a full tile of 16 and a half tile of 4
A_DIMS = [1, 3, 4, 5, 8, 12, 13, 16, 17, 20, 24, 28, 32, 33, 36, 48, 52, 64]
A_LENS, A_NQ, A_K = [5, 260, 1027], 20, 10
A_METRICS = [L2, IP]
assert {tail_of(d) for d in A_DIMS} == {4, 8, 12, 16}
assert {dp_of(d) for d in A_DIMS if dp_of(d) < 16} == {4, 8, 12}


@functools.lru_cache(maxsize=None)
def case_a(d, metric):
    rng = np.random.default_rng(100 + d)
    # at d = 1 the 10th L2 neighbour of a query inside a 1027-row cluster is
    # closer than 100 b (the cap fails on the reference; from d = 3 on it
    # holds): those queries are drawn away from the rows
    return make_case(1000 * d + metric, A_LENS, d, metric,
                     rng.integers(0, 3, A_NQ), scale=6.0, sigma=0.5,
                     qshift=2.0 if d == 1 else 0.0)


# B. d ladder: (d, metric, nq); nq = 9 is 9 of 16 (full body), 8 + 1 at
# QTM = 8, 4 + 4 + 1 at QTM = 4; nq = 8 at d = 2304 the half body at full LDS
B_QTM = {2304: 16, 2305: 8, 4608: 8, 4609: 4, 8189: 4, 8192: 4}
B_LENS, B_K = [3, 258], 10
B_CASES = [(d, m, 9) for d in B_QTM for m in (L2, IP)] + \
    [(2304, L2, 8), (2304, IP, 8), (4609, COSINE, 9)]
for _d, _t in B_QTM.items():
    assert qtm_of(_d) == _t, _d


@functools.lru_cache(maxsize=None)
def case_b(d, metric, nq):
    """At these dimensions one 4-dim group of evenly spread data moves a
    distance by 4 / d of itself, the size of the bound (d + 3) u.  The last
    4 dimensions therefore carry 16 times the noise of the others, so that
    a pipeline tail that loses its last group misses rule A by far."""
    rng = np.random.default_rng(200 + d + nq)
    return make_case(7 * d + metric + nq, B_LENS, d, metric,
                     rng.integers(0, 2, nq), scale=12.0, sigma=0.125,
                     edge_gain=16.0)


# C. wave, chunk and tile edges under partial probing (the tables of
# test_scan_fused_topk.py, restated)
C_LENS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 2049]
C_QPL = [1, 8, 9, 16, 17, 33, 1, 8, 17]
C_D = 32
C_FUSED = [(nprobe, k) for nprobe in (1, 3) for k in (1, 10, 64)]
C_STORE_ALL = [(3, 65), (9, 64)]  # by k, and by size: 9*3*4*64 > 5893
for _np, _k in C_FUSED:
    assert expect_fused(_k, _np, C_LENS)
for _np, _k in C_STORE_ALL:
    assert not expect_fused(_k, _np, C_LENS)
assert 9 * 3 * 4 * 64 == 6912 and sum(C_LENS) == 5893


@functools.lru_cache(maxsize=None)
def case_c(metric):
    return make_case(3000 + metric, C_LENS, C_D, metric,
                     np.repeat(np.arange(len(C_LENS)), C_QPL), scale=10.0,
                     sigma=0.3)


# D. filters, tombstones and upsert on the case C index, L2, nprobe = 3
D_NPROBE, D_KS = 3, (10, 65)
D_BITMAP_NBITS = 20000 + 37


def case_d_specs(c):
    """name -> filter spec (the dicts of flat_reference.filter_mask)."""
    ids = c.ids
    rng = np.random.default_rng(78)
    present = np.sort(rng.choice(ids, 900, replace=False))
    absent = np.array([0, 12, 13, 5 * 400 + 12, int(ids[-1]) + 1, 1 << 40],
                      np.int64)
    assert not np.isin(absent, ids).any()
    mixed = np.sort(np.concatenate([present, absent]))
    base = int(ids[300])
    words = (D_BITMAP_NBITS + 63) // 64
    bm = rng.integers(0, 1 << 63, words, dtype=np.uint64) << np.uint64(1)
    bm |= rng.integers(0, 2, words, dtype=np.uint64)
    bm[-1] |= ~np.uint64(0) << np.uint64(D_BITMAP_NBITS % 64)
    assert D_BITMAP_NBITS % 64 and (ids < base).any() and \
        (ids >= base + words * 64).any()
    # the last 40 rows of the 2049-row list in arrival order: if the atomic
    # cursor retires in order they are the end of its second chunk and the
    # single row of its third; nothing of any other list passes
    lo = int(ids[c.off[8] + 2049 - 40])
    return {
        "range": dict(kind=1, negate=False, min_id=int(ids[200]),
                      max_id=int(ids[4000])),
        "sorted_mixed": dict(kind=2, negate=False, ids=mixed),
        "bitmap": dict(kind=3, negate=False, bitmap=bm, bitmap_base=base,
                       bitmap_nbits=D_BITMAP_NBITS),
        "sorted_neg": dict(kind=2, negate=True, ids=mixed),
        "range_one_list": dict(kind=1, negate=False, min_id=lo,
                               max_id=int(ids[-1]) + 1),
    }


def case_d_victims(c, ref, elig):
    """Rows to remove: the whole 3-row list, the reference best eligible row
    of every fifth query, and the arrival-last row of a full chunk of the
    1024-, 1025- and 2049-row lists."""
    best = [int(np.nonzero(elig[i])[0][np.argmin(ref[i, elig[i]])])
            for i in range(0, ref.shape[0], 5)]
    edge = [int(c.off[6]) + 1023, int(c.off[7]) + 1023, int(c.off[8]) + 2047]
    short = list(range(int(c.off[1]), int(c.off[2])))
    return np.unique(np.array(short + best + edge))


def case_d_upsert(c, alive):
    """(rows, vectors): 8 live rows of the 2049-row list get vectors near
    the centroid of the 255-row list, each next to one of that list's
    queries so that it becomes the query's best row."""
    rng = np.random.default_rng(79)
    rows = np.nonzero(alive & (c.owner == 8))[0][5:800:100]
    assert len(rows) == 8
    near = c.q[np.nonzero(c.qlists == 2)[0][:8]]
    v = (near + 0.05 * rng.standard_normal((8, c.d))).astype(np.float32)
    return rows, v


# E. range search with partial probing: the default nprobe of 80 leaves 16 of
# 96 lists out
E_NLIST, E_D, E_NQ, E_BIG = 96, 32, 24, 40
E_LENS = [1030 if l == E_BIG else 26 + (7 * l) % 9 for l in range(E_NLIST)]
E_METRICS = [L2, IP]


@functools.lru_cache(maxsize=None)
def case_e(metric):
    rng = np.random.default_rng(500)
    return make_case(5000 + metric, E_LENS, E_D, metric,
                     rng.integers(0, E_NLIST, E_NQ), scale=10.0, sigma=0.3)


# F. graph replay on the case C index: nq <= 4 without a filter
F_NQS, F_K, F_NPROBE, F_CALLS = (1, 4), 10, 3, 4


def case_f_queries(c, nq, call):
    """Different queries for every call, near different centroids."""
    pick = (7 * call + 3 * np.arange(nq) + nq) % len(c.q)
    return np.ascontiguousarray(c.q[pick]), pick


# --------------------------------------------------------------------------
# the searches of every case group.  One driver per group runs in both test
# files: `ops` is the GPU index there and a dry run here (CPU), so the
# strength and ambiguity asserts, which need the reference alone, hold for
# exactly the searches the GPU file makes.
#   ops.search(where, q, k, nprobe, spec, ref, b, ids, elig, fused)
#   ops.range_search(where, q, radius, ref, b, ids, elig)
#   ops.remove(ids) / ops.upsert(ids, vectors)
#   ops.replayed(where, expected): was the last search a graph replay
# --------------------------------------------------------------------------
class DryOps:
    """The reference-only run of a driver."""
    def __init__(self):
        self.searches = 0

    def search(self, *a):
        self.searches += 1

    def range_search(self, *a):
        self.searches += 1

    def remove(self, ids):
        pass

    def upsert(self, ids, vectors):
        pass

    def replayed(self, where, expected):
        pass


def refb(c, q=None):
    """(ref, b) of the case's queries (cached) or of q."""
    if q is not None:
        return fr.ref_and_bound(c.metric, q, c.x)
    if not hasattr(c, "_refb"):
        c._refb = fr.ref_and_bound(c.metric, c.q, c.x)
    return c._refb


def topk(ops, c, where, q, k, nprobe, spec, ref, b, assign, alive,
         lens=None):
    """One top-k search of a driver: zero ambiguous probe sets, the strength
    cap, then the search itself.  Returns elig."""
    probed, amb = probe_sets(c.metric, q, c.cents, nprobe)
    assert len(amb) == 0, (where, "ambiguous probe set of queries", amb)
    elig = eligible(probed, assign,
                    alive & fr.filter_mask(spec, c.ids))
    fr.assert_topk_strength(c.metric, ref, b, elig, k, where)
    fused = expect_fused(k, nprobe, c.lens if lens is None else lens)
    ops.search(where, q, k, nprobe, spec, ref, b, c.ids, elig, fused)
    return elig


def run_full_probe(c, assign, ops, k_small):
    """Groups A and B: nprobe = nlist, k_small fused and k = N store-all,
    which reads out every (query, row) pair of the scan."""
    ref, b = refb(c)
    alive = np.ones(c.n, bool)
    assert expect_fused(k_small, c.nlist, c.lens)
    assert not expect_fused(c.n, c.nlist, c.lens)
    for k in (k_small, c.n):
        topk(ops, c, (c.metric, c.d, len(c.q), "k", k), c.q, k, c.nlist,
             None, ref, b, assign, alive)


def run_c(c, assign, ops):
    ref, b = refb(c)
    alive = np.ones(c.n, bool)
    for nprobe, k in C_FUSED + C_STORE_ALL:
        elig = topk(ops, c, (c.metric, "nprobe", nprobe, "k", k), c.q, k,
                    nprobe, None, ref, b, assign, alive)
        if nprobe == 1:  # lists shorter than k: rule D's padding
            short = elig.sum(1) < k
            assert short.any() == (k > 1) and not short.all()


def run_d(c, assign, ops):
    ref, b = refb(c)
    alive = np.ones(c.n, bool)
    specs = case_d_specs(c)
    one = fr.filter_mask(specs["range_one_list"], c.ids)
    assert one.sum() == 40 and (c.owner[one] == 8).all()
    probed, _ = probe_sets(c.metric, c.q, c.cents, D_NPROBE)
    for removed in (False, True):
        if removed:
            victims = case_d_victims(c, ref, eligible(probed, assign, alive))
            assert alive[victims].all() and len(victims) > 20
            ops.remove(c.ids[victims])
            alive[victims] = False
            assert not alive[c.owner == 1].any()
        for name, spec in list(specs.items()) + [("none", None)]:
            if removed and spec is not None:
                # the pass removes admissible rows of every kind but the
                # one-list range
                assert (fr.filter_mask(spec, c.ids) & ~alive).any() or \
                    name == "range_one_list"
            for k in D_KS:
                topk(ops, c, ("D", name, k, "removed", removed), c.q, k,
                     D_NPROBE, spec, ref, b, assign, alive)
    rows, vec = case_d_upsert(c, alive)
    ops.upsert(c.ids[rows], vec)
    x2 = c.x.copy()
    x2[rows] = vec
    ref2, b2 = fr.ref_and_bound(c.metric, c.q, x2)
    lens = list(c.lens)
    lens[2] += 8  # the new rows arrive in the 255-row list
    # nprobe = nlist: every list is probed, so where the new rows were
    # assigned does not enter the eligibility
    for k in D_KS:
        topk(ops, c, ("D", "upsert", k), c.q, k, c.nlist, None, ref2, b2,
             assign, alive, lens=lens)
    near = np.nonzero(c.qlists == 2)[0][:8]
    best = np.argmin(np.where(alive[None, :], ref2[near], np.inf), axis=1)
    assert np.array_equal(best, rows)  # each new vector is a query's best


def run_e(c, assign, ops):
    ref, b = refb(c)
    probed, amb = probe_sets(c.metric, c.q, c.cents, 0)
    assert len(amb) == 0 and (probed.sum(1) == DEFAULT_NPROBE).all()
    elig = eligible(probed, assign, np.ones(c.n, bool))
    radii = fr.range_radii(c.metric, ref, elig)
    fr.assert_range_strength(c.metric, radii, ref, b, elig)
    # a scan of every list would fail: rows of unprobed lists lie inside
    outside = False
    for radius in radii:
        must, _ = fr.range_reference(c.metric, float(np.float32(radius)),
                                     ref, b, np.ones(c.n, bool))
        outside |= bool((must & ~elig).any())
    assert outside
    for radius in radii:
        ops.range_search((c.metric, "radius", radius), c.q, radius, ref, b,
                         c.ids, elig)


def run_f(c, assign, ops, nq):
    """Four calls with different queries (the first runs and captures, the
    others replay), one remove, two more calls."""
    alive = np.ones(c.n, bool)
    ref_all, b_all = refb(c)
    seen = set()
    for call in range(F_CALLS + 2):
        if call == F_CALLS:
            # the best row of the next call's first query
            q, pick = case_f_queries(c, nq, call)
            probed, _ = probe_sets(c.metric, q, c.cents, F_NPROBE)
            e = eligible(probed, assign, alive)[0]
            victim = np.nonzero(e)[0][np.argmin(ref_all[pick[0], e])]
            ops.remove(c.ids[[victim]])
            alive[victim] = False
        q, pick = case_f_queries(c, nq, call)
        assert tuple(pick) not in seen
        seen.add(tuple(pick))
        topk(ops, c, ("F", nq, "call", call), q, F_K, F_NPROBE, None,
             ref_all[pick], b_all[pick], assign, alive)
        # the first call and the first after the remove run the kernels and
        # capture; every other call replays
        ops.replayed(("F", nq, "call", call), call not in (0, F_CALLS))
