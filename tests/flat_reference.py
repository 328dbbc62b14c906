"""float64 reference, error bound and acceptance rules for the Flat exact
path, the float range search and the float filters (test_flat_exact.py on
the GPU, test_flat_reference_cpu.py without one).

Reference, plain numpy float64 over the float32 inputs:
  L2      ||q - x||^2
  IP      q . x
  COSINE  qh . xh with qh = q / ||q||, xh = x / ||x|| normalised in f64
          (inputs keep ||.||^2 far from 1, so the "leave a row alone if
          |1 - n^2| <= 1e-5" rule of the normalisation kernel never applies)

Bound, derived from the design and not from any kernel's output.  The device
computes s = q . x, cn = ||x||^2 and qn = ||q||^2 as f32 sums of d products
each, then key = cn - 2 s and dist = key + qn.  With u = 2^-24 a length-d
f32 sum of products, in ANY summation order, is within d u sum|terms| of the
exact one (first order; the factor 2 is exact), and the two final
operations round once each against a magnitude of at most
qn + cn + 2 sum|q_i x_i|.  So, with d the caller's dimension (the internal
zero padding to a multiple of 4 adds exact zeros):

  b_L2(q, x)  = (d + 3) u (||q||^2 + ||x||^2 + 2 sum|q_i x_i|)
  b_IP(q, x)  = (d + 3) u sum|q_i x_i|
  b_COS(q, x) = (d + 9) u sum|qh_i xh_i|

The cosine bound carries 3 more roundings per stored component and 3 per
query component: norm^2 to f32, 1 / sqrt, and the scaling product.  Because
the bound holds for every summation order, one bound serves the hand MFMA
kernel, rocBLAS and the IVF-Flat scans.

Top-k acceptance (check_topk), every query of every search, no fraction may
be wrong; eligible = not removed and passing the filter:
  A  each returned (dist, id): |dist - ref(q, id)| <= b(q, id); for L2 the
     value 0.0 is also accepted when ref <= b (the emit clamps at 0);
  B  no eligible row that was left out beats a returned one by more than
     b(x) + b(y);
  C  returned distances are monotone, best first;
  D  exactly min(k, eligible) rows come back, distinct and eligible, the
     remaining slots are -1 / 0.0.
Strength (assert_topk_strength), on the reference alone: max b over the
eligible pairs is at most 1 % of the median over queries of |ref at rank
min(k, eligible)|, so A and B cannot pass vacuously.

Range acceptance (check_range): rows better than the radius by more than b
are present, rows worse by more than b are absent, rows in the band may go
either way; returned distances satisfy A; best first within a query with
ties toward the smaller id; lims consistent with the counts; and the
postcondition on the emitted f32 numbers, dist < radius (L2) / dist > radius
(IP, COSINE).  Strength (assert_range_strength): at most 5 % of the eligible
pairs lie in the band at each radius, and over the radii of a case the
reference has a non-empty answer and one that is neither empty nor the
whole eligible set.

The input generators and the shape tables live here so that the CPU file
asserts the strength conditions for exactly the inputs the GPU file uses.
"""
import numpy as np

L2, IP, COSINE = 0, 1, 2
U = 2.0 ** -24
TOPK_CAP = 0.01
BAND_CAP = 0.05

# largest observed |dist - ref| / b per metric, kept for the record
MAX_RATIO = {L2: 0.0, IP: 0.0, COSINE: 0.0}


# --------------------------------------------------------------------------
# reference values and bound
# --------------------------------------------------------------------------
def ref_and_bound(metric, q32, x32):
    """(ref, b), both float64 [nq, n]."""
    q = np.asarray(q32, np.float32).astype(np.float64)
    x = np.asarray(x32, np.float32).astype(np.float64)
    d = q.shape[1]
    if metric == COSINE:
        q = q / np.sqrt((q * q).sum(1, keepdims=True))
        x = x / np.sqrt((x * x).sum(1, keepdims=True))
    dot = q @ x.T
    adot = np.abs(q) @ np.abs(x).T
    if metric == L2:
        qn = (q * q).sum(1)[:, None]
        xn = (x * x).sum(1)[None, :]
        ref = np.maximum(qn + xn - 2.0 * dot, 0.0)
        # exact value from the differences where cancellation would cost
        # f64 digits (queries equal to stored rows)
        small = ref < 1e-6 * (qn + xn)
        if small.any():
            qi, xi = np.nonzero(small)
            ref[qi, xi] = ((q[qi] - x[xi]) ** 2).sum(1)
        return ref, (d + 3) * U * (qn + xn + 2.0 * adot)
    if metric == IP:
        return dot, (d + 3) * U * adot
    return dot, (d + 9) * U * adot


def better_sign(metric):
    """+1 if smaller is better (L2), -1 if larger is (IP, COSINE)."""
    return 1.0 if metric == L2 else -1.0


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def gaussian(seed, nq, n, d, metric=L2):
    """(queries, rows) float32, Gaussian; COSINE inputs are scaled so that
    squared norms sit near 9 d (and 4 d), far from 1."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    if metric == COSINE:
        x *= np.float32(3.0)
        q *= np.float32(2.0)
        assert ((x.astype(np.float64) ** 2).sum(1) > 1.5).all()
        assert ((q.astype(np.float64) ** 2).sum(1) > 1.5).all()
    return q, x


# Which GEMM serves dots[rows x cols] over the padded dimension dp =
# ceil(d / 4) * 4 (sgemm_dots): the hand MFMA kernel for rows <= 8, or for
# rows >= 48 and 64 <= cols <= 16384 and dp >= 64; rocBLAS otherwise.
def gemm_route(nq, n, d):
    dp = (d + 3) // 4 * 4
    if nq <= 8:
        return "mfma_latency"
    if nq >= 48 and 64 <= n <= 16384 and dp >= 64:
        return "mfma_tile"
    return "rocblas"


# (nq, N, d).  The hand kernel works in 128 x 128 x 32 tiles: nq and N cover
# a partial M block, a partial N block, exact blocks and a second partial
# block; after the pad to a multiple of 4, K = 68 has both staging halves of
# the last step on the element-wise path, 80 one half on the float4 path and
# one on the edge path, 84 a 4-of-16 half, 64 and 96 exact steps.  Every
# listed value of an axis occurs with at least two values of the others.
GEMM_TILE_SHAPES = [
    (48, 64, 64), (48, 300, 65), (48, 128, 80),
    (127, 127, 80), (127, 129, 100),
    (128, 128, 96), (128, 64, 84), (128, 300, 100),
    (129, 129, 65), (129, 300, 64),
    (200, 300, 84), (200, 127, 96),
]
GEMM_LATENCY_SHAPES = [
    (1, 1, 1), (1, 5, 33), (1, 63, 128), (1, 129, 4), (1, 63, 12),
    (3, 1, 12), (3, 5, 1), (3, 63, 4), (3, 129, 128),
    (8, 1, 128), (8, 5, 12), (8, 63, 33), (8, 129, 1), (8, 129, 33),
]
GEMM_ROCBLAS_SHAPES = [(20, 300, 64), (64, 300, 32)]
GEMM_COSINE_SHAPES = [(128, 128, 96), (129, 300, 65)]
for _s in GEMM_TILE_SHAPES + GEMM_COSINE_SHAPES:
    assert gemm_route(*_s) == "mfma_tile", _s
for _s in GEMM_LATENCY_SHAPES:
    assert gemm_route(*_s) == "mfma_latency", _s
for _s in GEMM_ROCBLAS_SHAPES:
    assert gemm_route(*_s) == "rocblas", _s

# selector edges: (N, k), nq = 4, d = 16.  The dense select runs 8 column
# segments of ceil(N / 8): N = 5 leaves three of them empty, N = 9 gives the
# last ones a width of 1 and -1.  The library caps k at 2048, so N = 3000
# runs k = 2048 in the place of k = N and k = N + 3.
SELECT_SMALL = [(n, k) for n in (5, 9, 64) for k in (1, 10, n, n + 3)] + \
    [(3000, 1), (3000, 10), (3000, 2048)]
# block shrink (select_threads: 16 threads at k = 300, 4 at k = 2048); at
# k = 2048 each segment of ceil(2500 / 8) = 313 columns returns fewer than k
SELECT_WIDE = [(2500, k) for k in (129, 300, 1024, 2048)]
SELECT_D = 16

DUP_N, DUP_D = 2500, 32
DUP_ROWS = np.array([10, 333, 944, 1352, 1885, 2491])  # segments 0 1 3 4 6 7


def gemm_seed(nq, n, d):
    return 1000003 * nq + 1009 * n + d


def select_seed(n):
    return 5000 + n


def duplicates_case(nq):
    """(queries, rows, DUP_ROWS): six exact copies of one vector in
    different column segments (width ceil(2500 / 8) = 313), every query
    close to it so that the copies are its six nearest rows."""
    assert (np.diff(DUP_ROWS // 313) > 0).all()
    rng = np.random.default_rng(4242)
    x = rng.standard_normal((DUP_N, DUP_D)).astype(np.float32)
    x[DUP_ROWS] = x[DUP_ROWS[0]]
    q = (x[DUP_ROWS[0]][None, :] +
         0.05 * rng.standard_normal((nq, DUP_D))).astype(np.float32)
    return q, x, DUP_ROWS


# multi-chunk Flat: nchunks > 1 needs N > max(65536, 2^29 / nq)
MC_NQ, MC_N, MC_D, MC_K, MC_SAMPLES = 8192, 65536 + 64, 8, 10, 64
MC_SEED = 8192
MC_CHUNK = 65536


def multichunk_samples():
    """The fully checked query rows: first, last and 62 random ones."""
    rng = np.random.default_rng(MC_SEED + 1)
    mid = rng.choice(np.arange(1, MC_NQ - 1), MC_SAMPLES - 2, replace=False)
    return np.sort(np.concatenate([[0, MC_NQ - 1], mid]))


def multichunk_data(metric):
    """Gaussian queries and rows; three rows of the 64-column second chunk
    are planted as the best match of three sampled queries (a copy of the
    query plus noise; scaled up for IP so that the score wins)."""
    q, x = gaussian(MC_SEED, MC_NQ, MC_N, MC_D, metric)
    rng = np.random.default_rng(MC_SEED + 2)
    rows = multichunk_samples()
    for j in range(3):
        v = q[rows[5 + 7 * j]] * np.float32(1.0 if metric == L2 else 6.0)
        x[MC_CHUNK + 3 + 25 * j] = v + (
            0.1 * rng.standard_normal(MC_D)).astype(np.float32)
    return q, x


def multichunk_victims(metric, ref):
    """Six rows to remove: the reference nearest neighbours of three sampled
    queries that lie in the first chunk and of three in the second.  ref is
    the reference of the sampled queries."""
    best = np.argmin(better_sign(metric) * ref, axis=1)
    first = np.unique(best[best < MC_CHUNK])[:3]
    second = np.unique(best[best >= MC_CHUNK])[:3]
    return np.concatenate([first, second])


def kth_radius(metric, ref, elig, kth):
    """Median over the queries of the kth best eligible reference value,
    as the float32 the caller hands to range search."""
    sg = better_sign(metric)
    e = elig if elig.ndim == 2 else np.broadcast_to(elig, ref.shape)
    vals = [np.sort(sg * ref[i, e[i]])[kth - 1] * sg
            for i in range(ref.shape[0]) if e[i].sum() >= kth]
    return float(np.float32(np.median(vals)))


def range_radii(metric, ref, elig):
    """[median 5th neighbour, a radius that returns nothing, one that
    returns every eligible row], float32 values.  elig is bool [n] or
    [nq, n]."""
    sg = better_sign(metric)
    s = sg * (ref[:, elig] if elig.ndim == 1 else ref[elig])
    lo, hi = s.min(), s.max()
    nothing = 0.5 * lo if metric == L2 else sg * (lo - 0.25 * (hi - lo))
    everything = sg * (hi + 0.25 * (hi - lo))
    return [kth_radius(metric, ref, elig, 5), float(np.float32(nothing)),
            float(np.float32(everything))]


# filters
FILT_N, FILT_D, FILT_NQ = 3000, 32, 16
FILT_SEED = 3000
BITMAP_BASE, BITMAP_NBITS = 1000, 8000 + 37


def filter_victims():
    """Rows removed for the second pass of the filter matrix: 300 random
    ones plus the only admissible row of `sorted_single` and one of the four
    of `sorted_few`."""
    ids = filter_ids()
    specs = filter_specs()
    rng = np.random.default_rng(FILT_SEED + 1)
    rows = rng.choice(FILT_N, 300, replace=False)
    extra = np.nonzero(np.isin(ids, [specs["sorted_single"]["ids"][0],
                                     specs["sorted_few"]["ids"][1]]))[0]
    return np.unique(np.concatenate([rows, extra]))


def self_query_rows():
    return np.random.default_rng(FILT_SEED + 2).choice(FILT_N, FILT_NQ,
                                                       replace=False)


def filter_ids():
    """3000 ascending, non-contiguous ids; the last 1000 lie above 2^33."""
    lo = 7 * np.arange(2000, dtype=np.int64) + 3
    hi = (1 << 33) + 11 * np.arange(1000, dtype=np.int64) + 5
    return np.concatenate([lo, hi])


def filter_specs():
    """name -> spec dict (kind, negate and the kind's fields).  Kinds are
    the dg_filter_kind values: 1 RANGE, 2 SORTED_IDS, 3 BITMAP."""
    ids = filter_ids()
    rng = np.random.default_rng(77)
    present = np.sort(rng.choice(ids, 400, replace=False))
    absent = np.array([0, 4, 11, 14001, (1 << 33) + 6, (1 << 40)], np.int64)
    assert not np.isin(absent, ids).any()
    mixed = np.sort(np.concatenate([present, absent]))
    words = (BITMAP_NBITS + 63) // 64
    bm = rng.integers(0, 1 << 63, words, dtype=np.uint64) << np.uint64(1)
    bm |= rng.integers(0, 2, words, dtype=np.uint64)
    # bits past nbits in the last word are SET: they must not admit anything
    bm[-1] |= ~np.uint64(0) << np.uint64(BITMAP_NBITS % 64)
    assert (ids < BITMAP_BASE).any()
    last_word = (ids >= BITMAP_BASE + BITMAP_NBITS) & \
        (ids < BITMAP_BASE + words * 64)
    assert last_word.any() and (ids >= BITMAP_BASE + words * 64).any()
    lo, hi = int(ids[500]), int(ids[2500]) + 1  # spans the 2^33 jump
    bmf = dict(bitmap=bm, bitmap_base=BITMAP_BASE, bitmap_nbits=BITMAP_NBITS)
    return {
        "range": dict(kind=1, negate=False, min_id=lo, max_id=hi),
        "range_neg": dict(kind=1, negate=True, min_id=lo, max_id=hi),
        "range_empty": dict(kind=1, negate=False, min_id=lo, max_id=lo),
        "sorted_mixed": dict(kind=2, negate=False, ids=mixed),
        "sorted_single": dict(kind=2, negate=False, ids=present[200:201]),
        "sorted_neg": dict(kind=2, negate=True, ids=mixed),
        "bitmap": dict(kind=3, negate=False, **bmf),
        "bitmap_neg": dict(kind=3, negate=True, **bmf),
        "sorted_few": dict(kind=2, negate=False, ids=present[[3, 90, 250,
                                                              399]]),
    }


def filter_mask(spec, ids):
    """bool [len(ids)]: the ids the filter admits (the reference model)."""
    ids = np.asarray(ids, np.int64)
    if spec is None:
        return np.ones(len(ids), bool)
    if spec["kind"] == 1:
        inside = (ids >= spec["min_id"]) & (ids < spec["max_id"])
    elif spec["kind"] == 2:
        inside = np.isin(ids, spec["ids"])
    else:
        bit = ids - spec["bitmap_base"]
        ok = (bit >= 0) & (bit < spec["bitmap_nbits"])
        b = np.where(ok, bit, 0)
        word = spec["bitmap"][b >> 6]
        inside = ok & (((word >> (b & 63).astype(np.uint64)) &
                        np.uint64(1)) == 1)
    return ~inside if spec["negate"] else inside


# --------------------------------------------------------------------------
# checkers
# --------------------------------------------------------------------------
def _rows_of(ids_sorted, sorter, got, where):
    pos = np.searchsorted(ids_sorted, got)
    pos = np.minimum(pos, len(ids_sorted) - 1)
    assert (ids_sorted[pos] == got).all(), (where, "unknown id", got)
    return sorter[pos]


def _elig_rows(elig, qi):
    return elig[qi] if elig.ndim == 2 else elig


def assert_topk_strength(metric, ref, b, elig, k, where=""):
    """The cap that keeps A and B from passing vacuously; reference only."""
    at_rank, bmax = [], 0.0
    for qi in range(ref.shape[0]):
        e = _elig_rows(elig, qi)
        m = min(k, int(e.sum()))
        if m == 0:
            continue
        key = np.sort(better_sign(metric) * ref[qi, e])
        at_rank.append(abs(key[m - 1]))
        bmax = max(bmax, b[qi, e].max())
    if not at_rank:
        return 0.0
    scale = float(np.median(at_rank))
    assert bmax <= TOPK_CAP * scale, (where, "bound too weak", bmax, scale)
    return bmax / scale


def check_topk(metric, dist, ids, ref, b, row_ids, elig, where=""):
    """Checks A-D of one search; ref/b are [nq, n] over the rows row_ids,
    elig is bool [n] or [nq, n].  Returns the largest |dist - ref| / b."""
    dist = np.asarray(dist)
    ids = np.asarray(ids)
    nq, k = ids.shape
    assert dist.shape == (nq, k) and ref.shape[0] == nq
    sorter = np.argsort(row_ids, kind="stable")
    ids_sorted = np.asarray(row_ids)[sorter]
    sg = better_sign(metric)
    worst = 0.0
    for qi in range(nq):
        w = (where, "query", qi)
        e = _elig_rows(elig, qi)
        m = min(k, int(e.sum()))
        # D
        assert (ids[qi, m:] == -1).all(), (w, "padding ids", ids[qi, m:])
        assert (dist[qi, m:] == 0.0).all(), (w, "padding dist", dist[qi, m:])
        got = ids[qi, :m]
        assert (got >= 0).all(), (w, "too few rows", got)
        rows = _rows_of(ids_sorted, sorter, got, w)
        assert len(np.unique(rows)) == m, (w, "duplicate rows", got)
        assert e[rows].all(), (w, "ineligible row", got[~e[rows]])
        if m == 0:
            continue
        # A
        dd = dist[qi, :m].astype(np.float64)
        r, bb = ref[qi, rows], b[qi, rows]
        err = np.abs(dd - r)
        ok = err <= bb
        if metric == L2:
            ok |= (dd == 0.0) & (r <= bb)
        assert ok.all(), (w, "distance off", got[~ok], dd[~ok], r[~ok],
                          bb[~ok])
        fin = (err <= bb) & (bb > 0)
        worst = max(worst, float((err[fin] / bb[fin]).max(initial=0.0)))
        # C
        assert (np.diff(sg * dist[qi, :m]) >= 0).all(), (w, "not monotone")
        # B
        left = e.copy()
        left[rows] = False
        if left.any():
            best_left = (sg * ref[qi, left] + b[qi, left]).min()
            worst_got = (sg * r - bb).max()
            assert best_left >= worst_got, (w, "better row left out",
                                            best_left, worst_got)
    MAX_RATIO[metric] = max(MAX_RATIO[metric], worst)
    return worst


def range_reference(metric, radius, ref, b, elig):
    """(must, may): bool [nq, n], rows that have to be present and rows that
    may be (must plus the band)."""
    sg = better_sign(metric)
    e = elig if elig.ndim == 2 else np.broadcast_to(elig, ref.shape)
    must = e & (sg * ref < sg * radius - b)
    may = e & (sg * ref <= sg * radius + b)
    return must, may


def assert_range_strength(metric, radii, ref, b, elig, where=""):
    """Per radius at most BAND_CAP of the eligible pairs in the band; over
    the radii of the case one non-empty reference answer and one that is
    neither empty nor everything."""
    e = elig if elig.ndim == 2 else np.broadcast_to(elig, ref.shape)
    npairs = int(e.sum())
    nonempty = nontrivial = False
    for radius in radii:
        must, may = range_reference(metric, float(radius), ref, b, elig)
        band = int((may & ~must).sum())
        assert band <= BAND_CAP * npairs, (where, radius, "band too wide",
                                           band, npairs)
        cnt, tot = must.sum(1), e.sum(1)
        nonempty |= bool((cnt > 0).any())
        nontrivial |= bool(((cnt > 0) & (may.sum(1) < tot)).any())
    assert nonempty and nontrivial, (where, "degenerate radii", radii)


def check_range(metric, radius, lims, dist, ids, ref, b, row_ids, elig,
                where="", queries=None):
    """Range acceptance for the queries `queries` (default all; ref/b/elig
    rows correspond to them in order).  Returns the largest |dist-ref|/b."""
    lims = np.asarray(lims)
    dist = np.asarray(dist)
    ids = np.asarray(ids)
    assert dist.dtype == np.float32
    assert lims[0] == 0 and (np.diff(lims) >= 0).all(), (where, "lims")
    assert lims[-1] == len(dist) == len(ids), (where, "lims vs sizes")
    if queries is None:
        queries = np.arange(len(lims) - 1)
    assert len(queries) == ref.shape[0]
    sorter = np.argsort(row_ids, kind="stable")
    ids_sorted = np.asarray(row_ids)[sorter]
    sg = better_sign(metric)
    rad32 = np.float32(radius)
    must, may = range_reference(metric, float(rad32), ref, b, elig)
    worst = 0.0
    for j, qi in enumerate(queries):
        w = (where, "radius", radius, "query", int(qi))
        a, z = int(lims[qi]), int(lims[qi + 1])
        got, dd32 = ids[a:z], dist[a:z]
        # postcondition on the emitted f32 numbers
        bad = ~(dd32 < rad32) if metric == L2 else ~(dd32 > rad32)
        assert not bad.any(), (w, "dist on the wrong side of the radius",
                               got[bad], dd32[bad])
        rows = _rows_of(ids_sorted, sorter, got, w)
        assert len(np.unique(rows)) == len(rows), (w, "duplicate rows")
        assert may[j, rows].all(), (w, "row beyond the radius or ineligible",
                                    got[~may[j, rows]])
        present = np.zeros(ref.shape[1], bool)
        present[rows] = True
        assert present[must[j]].all(), (
            w, "row within the radius missing",
            np.asarray(row_ids)[must[j] & ~present])
        if len(rows) == 0:
            continue
        dd = dd32.astype(np.float64)
        r, bb = ref[j, rows], b[j, rows]
        err = np.abs(dd - r)
        ok = err <= bb
        if metric == L2:
            ok |= (dd == 0.0) & (r <= bb)
        assert ok.all(), (w, "distance off", got[~ok], dd[~ok], r[~ok])
        fin = (err <= bb) & (bb > 0)
        worst = max(worst, float((err[fin] / bb[fin]).max(initial=0.0)))
        # best first, ties toward the smaller id
        key = sg * dd32
        step = np.diff(key)
        assert (step >= 0).all(), (w, "not best first")
        tie = step == 0
        assert (np.diff(got)[tie] > 0).all(), (w, "tie order")
    MAX_RATIO[metric] = max(MAX_RATIO[metric], worst)
    return worst
