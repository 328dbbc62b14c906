"""IVF-PQ encode pipeline + ADC scan against a float64 reference (marked gpu).

Inputs are built so that every row's list and PQ codes are known by
construction: well separated centroids, fixed-seed codebooks whose codewords
keep a minimum distance, and x = c_l + concat_m cb[m][code_m] + noise with
the noise far below that distance.  Each case asserts in f64 that the
constructed codeword (per subspace) and centroid win by at least 10x the
noise, so the GPU coarse assignment and encoder have one right answer and a
wrong code byte shows up as a wrong distance.

Reference: ||q - (c_l + cb[codes])||^2 in f64 (q . (c_l + cb[codes]) for IP,
the same on normalized inputs for COSINE).

Tolerance, derived from the design and not from the kernel's output: beyond
f32 the design rounds each S and T table entry once to f16 (relative 2^-11),

  b_L2(q,row) = 2^-11 * sum_m(|S_m| + 2|T_m|) + acc,
  b_IP(q,row) = 2^-11 * sum_m |T_m|           + acc,

with S_m = ||c_sub + cb_m[code_m]||^2, T_m = q_sub . cb_m[code_m] from the
f64 tables and acc = (M + 3) * 2^-24 * (sum of the magnitudes added, with
||q||^2 and 2|q.c| for L2, |q.c| for IP).  f16 subnormals (|T| < 6.1e-5)
round with absolute error 2^-25, which acc covers many times over at these
magnitudes.

Every query of every search is checked (no fraction may be wrong):
  A  each returned (dist, id) has |dist - ref(q, id)| <= b(q, id);
  B  no eligible row that was left out beats a returned one by more than
     the two bounds: ref(x) - ref(y) >= -(b(x) + b(y));
  C  returned distances are monotone;
  D  exactly min(k, eligible) rows come back, distinct and eligible, and the
     remaining slots are -1 / 0.0.
Each case also asserts, on the reference alone, that max b is at most 5 % of
the median k-th reference distance, so that A and B cannot pass vacuously.

Geometry: the scan stages 256-row tiles (RPV=4 x 64 lanes) of 1024-row
chunks and splits a list's probing queries over 4 waves.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "dingo-store_amd")]

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")

HALF_MAX = 65504.0
EPS16 = 2.0 ** -11
EPS32 = 2.0 ** -24
A_CENT = 6.0  # centroid norm in units of the codebook box side

# one row, under a wave, around the 256-row tile, around the 1024-row chunk,
# a third chunk of one row
LENS = [1, 3, 255, 256, 257, 1023, 1024, 1025, 2049]
# queries per list at nprobe=1 over 4 waves: one wave busy, all four, a
# second round of one, two full rounds, a third round
QPL = [1, 4, 5, 8, 9, 1, 4, 5, 9]


def _separated_box(rng, dim, sep):
    """256 points of [-0.5, 0.5]^dim, pairwise at least sep apart."""
    pts = np.empty((256, dim))
    n = 0
    while n < 256:
        c = rng.uniform(-0.5, 0.5, dim)
        if n == 0 or np.sqrt(((pts[:n] - c) ** 2).sum(1)).min() >= sep:
            pts[n] = c
            n += 1
    return pts


def _separated_sphere(rng, sep):
    """256 unit vectors of R^3, pairwise at least sep apart."""
    pts = np.empty((256, 3))
    n = 0
    while n < 256:
        c = rng.normal(size=3)
        c /= np.linalg.norm(c)
        if n == 0 or np.sqrt(((pts[:n] - c) ** 2).sum(1)).min() >= sep:
            pts[n] = c
            n += 1
    return pts


class Case:
    """Centroids, codebooks, rows with known (list, codes), and the f64
    model of the index: ids / lists / codes / alive of every row added."""

    def __init__(self, metric, d, m, nlist, seed, scale=1.0):
        self.metric, self.d, self.m, self.nlist = metric, d, m, nlist
        self.dsub = dsub = d // m
        self.scale = scale
        self.rng = rng = np.random.default_rng(seed)
        cents = np.zeros((nlist, d))
        cb = np.empty((m, 256, dsub))
        if metric == dg.COSINE:
            # unit-norm rows by construction: centroids on +-axis 0 of the
            # subspaces, codewords orthogonal to those axes and of one norm
            # rho, A^2 + m * rho^2 = 1
            assert dsub == 4 and nlist <= 2 * m and scale == 1.0
            rho = 0.3 / np.sqrt(m)
            self.A = np.sqrt(1.0 - m * rho * rho)
            for l in range(nlist):
                cents[l, dsub * (l % m)] = self.A if l < m else -self.A
            self.sep = 0.1 * rho
            bases = [_separated_sphere(rng, 0.1) * rho for _ in range(4)]
            for j in range(m):
                cb[j, :, 0] = 0.0
                cb[j, :, 1:] = bases[j % 4][rng.permutation(256)]
        else:
            assert nlist <= d
            self.A = A_CENT * scale
            cents[np.arange(nlist), np.arange(nlist)] = self.A
            sep0 = 0.25 * 256.0 ** (-1.0 / dsub)
            self.sep = sep0 * 0.8 * scale
            bases = [_separated_box(rng, dsub, sep0) for _ in range(4)]
            for j in range(m):  # permuted, mirrored, rescaled copies
                cb[j] = (bases[j % 4][rng.permutation(256)] *
                         rng.choice([-1.0, 1.0], dsub) *
                         rng.uniform(0.8, 1.0) * scale)
        self.noise = self.sep / 40.0
        self.cents32 = cents.astype(np.float32)
        self.cb32 = cb.astype(np.float32)
        self.C = self.cents32.astype(np.float64)
        self.CB = self.cb32.astype(np.float64)
        self.ids = np.empty(0, np.int64)
        self.lists = np.empty(0, np.int64)
        self.codes = np.empty((0, m), np.uint8)
        self.alive = np.empty(0, bool)
        # index-static table, f64: S[l][m][code]
        cs = self.C.reshape(nlist, m, 1, dsub)
        self.S = ((cs + self.CB[None]) ** 2).sum(-1)
        assert self.S.max() < HALF_MAX or scale != 1.0

    # ---- construction -------------------------------------------------
    def residuals(self, codes):
        return self.CB[np.arange(self.m)[None, :], codes].reshape(
            len(codes), self.d)

    def make_rows(self, lists):
        """Rows of the given lists with random codes; asserts in f64 that
        the construction is unambiguous.  Returns (codes, x float32)."""
        rng, n = self.rng, len(lists)
        codes = rng.integers(0, 256, (n, self.m)).astype(np.uint8)
        nz = rng.normal(size=(n, self.m, self.dsub))
        nz *= (self.noise * rng.uniform(0.2, 1.0, (n, self.m, 1)) /
               np.linalg.norm(nz, axis=2, keepdims=True))
        y = self.C[lists] + self.residuals(codes) + nz.reshape(n, self.d)
        if self.metric == dg.COSINE:  # the index normalizes what it is given
            y *= rng.uniform(0.5, 2.0, (n, 1))
        x32 = np.ascontiguousarray(y, np.float32)
        self.assert_unambiguous(lists, codes, x32)
        return codes, x32

    def _unit(self, v):
        v = np.asarray(v, np.float64)
        if self.metric == dg.COSINE:
            v = v / np.linalg.norm(v, axis=-1, keepdims=True)
        return v

    def assert_unambiguous(self, lists, codes, x32):
        X = self._unit(x32)
        n, m, dsub = len(X), self.m, self.dsub
        res = (X - self.C[lists]).reshape(n, m, dsub)
        nz = np.linalg.norm(res - self.CB[np.arange(m)[None, :], codes],
                            axis=2)  # [n, m] actual noise per subspace
        nz_row = np.sqrt((nz ** 2).sum(1))
        if self.metric == dg.L2:
            key = np.sqrt(((X[:, None, :] - self.C[None]) ** 2).sum(-1))
        else:  # larger dot wins; in units of length along the centroid
            key = -(X @ self.C.T) / self.A
        if self.nlist > 1:
            part = np.partition(key, 1, axis=1)
            assert (key.argmin(1) == lists).all()
            assert (part[:, 1] - part[:, 0] >= 10 * nz_row).all()
        step = max(1, 4_000_000 // (m * 256))
        cbn = (self.CB ** 2).sum(-1)  # [m, 256]
        for s in range(0, n, step):
            r = res[s:s + step]
            d2 = ((r ** 2).sum(-1)[:, :, None] + cbn[None] -
                  2 * np.einsum("nmd,mkd->nmk", r, self.CB))
            dist = np.sqrt(np.maximum(d2, 0.0))
            assert (dist.argmin(2) == codes[s:s + step]).all()
            part = np.partition(dist, 1, axis=2)
            assert (part[:, :, 1] - part[:, :, 0] >=
                    10 * nz[s:s + step]).all()

    def record(self, ids, lists, codes):
        ids = np.asarray(ids, np.int64)
        self.alive[np.isin(self.ids, ids)] = False  # upsert semantics
        self.ids = np.concatenate([self.ids, ids])
        self.lists = np.concatenate([self.lists, lists])
        self.codes = np.concatenate([self.codes, codes])
        self.alive = np.concatenate([self.alive, np.ones(len(ids), bool)])

    def forget(self, ids):
        self.alive[np.isin(self.ids, ids)] = False

    def new_index(self):
        idx = dg.Index(dg.IVF_PQ, self.metric, self.d, nlist=self.nlist,
                       m=self.m)
        idx.set_centroids(self.cents32)
        idx.set_codebooks(self.cb32)
        return idx

    def queries(self, lists, spread=0.5):
        """A query near the centroid of each given list."""
        u = self.rng.uniform(-spread, spread, (len(lists), self.d))
        if self.metric == dg.COSINE:
            u *= 0.3 / np.sqrt(self.d / 12.0)
            q = (self.C[lists] + u) * self.rng.uniform(0.5, 2.0,
                                                       (len(lists), 1))
        else:
            q = self.C[lists] + u * self.scale
        return np.ascontiguousarray(q, np.float32)

    # ---- reference ----------------------------------------------------
    def coarse_keys(self, q):
        """f64 coarse key of one (normalized) query per list, smaller is
        nearer."""
        if self.metric == dg.L2:
            return ((q[None] - self.C) ** 2).sum(1)
        return -(self.C @ q)

    def reference(self, q):
        """(key, b, dist) over all model rows for one query: key orders
        (smaller is better), dist is what the index reports."""
        n, m, dsub = len(self.ids), self.m, self.dsub
        R = self.residuals(self.codes)
        c = self.C[self.lists]
        Y = c + R
        T = (q.reshape(1, m, dsub) * R.reshape(n, m, dsub)).sum(-1)
        sum_t = np.abs(T).sum(1)
        qc = np.abs(c @ q)
        if self.metric == dg.L2:
            dist = ((q[None] - Y) ** 2).sum(1)
            sum_s = (Y ** 2).sum(1)  # sum_m S_m, all terms >= 0
            mag = sum_s + 2 * sum_t
            b = EPS16 * mag + (m + 3) * EPS32 * (mag + q @ q + 2 * qc)
            return dist, b, dist
        dist = Y @ q
        b = EPS16 * sum_t + (m + 3) * EPS32 * (sum_t + qc)
        return -dist, b, dist

    def check(self, q32, k, nprobe, gd, gi, keep=None, mask=None,
              min_gap=None):
        """Checks A-D for every query and the 5 % strength condition.
        keep: predicate on an id array (the filter); mask: list mask."""
        Q = self._unit(q32)
        # T stays inside f16 for these queries (f64 tables)
        tq = np.einsum("qmd,mkd->qmk", Q.reshape(len(Q), self.m, self.dsub),
                       self.CB)
        assert np.abs(tq).max() < HALF_MAX
        assert gd.shape == gi.shape == (len(Q), k)
        passes = self.alive.copy()
        if keep is not None:
            passes &= keep(self.ids)
        kth, bmax = [], 0.0
        for r, q in enumerate(Q):
            ck = self.coarse_keys(q)
            order = np.argsort(ck, kind="stable")
            if nprobe < self.nlist:  # the probe set itself must be clear
                gap = ck[order[nprobe]] - ck[order[nprobe - 1]]
                assert gap >= (min_gap if min_gap is not None
                               else 1e-3 * self.A * self.A), (r, gap)
            probed = np.zeros(self.nlist, bool)
            probed[order[:nprobe]] = True
            if mask is not None:
                probed &= mask.astype(bool)
            elig = passes & probed[self.lists]
            key, b, dist = self.reference(q)
            n_ret = min(k, int(elig.sum()))
            # D
            assert (gi[r, :n_ret] >= 0).all(), (r, gi[r])
            assert (gi[r, n_ret:] == -1).all(), (r, gi[r])
            assert (gd[r, n_ret:] == 0.0).all(), (r, gd[r])
            if n_ret == 0:
                continue
            cand = np.nonzero(elig)[0]
            by_id = dict(zip(self.ids[cand].tolist(), cand.tolist()))
            assert len(by_id) == len(cand)
            got = gi[r, :n_ret].tolist()
            assert len(set(got)) == n_ret, (r, got)
            assert all(g in by_id for g in got), (r, got)
            rows = np.array([by_id[g] for g in got])
            # A
            err = np.abs(gd[r, :n_ret].astype(np.float64) - dist[rows])
            assert (err <= b[rows]).all(), (r, err, b[rows])
            # B
            rest = np.setdiff1d(cand, rows)
            if len(rest):
                assert ((key[rest] + b[rest]).min() >=
                        (key[rows] - b[rows]).max()), r
            # C
            step = np.diff(gd[r, :n_ret])
            assert (step >= 0).all() if self.metric == dg.L2 else \
                (step <= 0).all(), (r, gd[r])
            kth.append(abs(np.sort(key[cand])[n_ret - 1]))
            bmax = max(bmax, b[cand].max())
        if kth:
            assert bmax <= 0.05 * np.median(kth), (bmax, np.median(kth))


def _grouped_case(metric, d, m, lens, seed, scale=1.0):
    """Rows list by list, id == position."""
    case = Case(metric, d, m, len(lens), seed, scale)
    lists = np.repeat(np.arange(len(lens)), lens)
    codes, x32 = case.make_rows(lists)
    return case, lists, codes, x32


def _add_all(case, idx, lists, codes, x32, ids=None):
    ids = np.arange(len(lists), dtype=np.int64) if ids is None else ids
    idx.add(ids, x32)
    case.record(ids, lists, codes)


_CACHE = {}


@pytest.fixture(scope="module")
def lens_index():
    """The LENS geometry per metric, built on first use and never mutated."""
    def get(metric):
        if metric not in _CACHE:
            case, lists, codes, x32 = _grouped_case(metric, 32, 8, LENS,
                                                    1000 + metric)
            idx = case.new_index()
            _add_all(case, idx, lists, codes, x32)
            q_one = case.queries(np.repeat(np.arange(len(LENS)), QPL))
            q_all = case.queries(case.rng.integers(0, len(LENS), 33))
            _CACHE[metric] = (case, idx, q_one, q_all)
        return _CACHE[metric]
    yield get
    for _, idx, _, _ in _CACHE.values():
        idx.close()
    _CACHE.clear()


def _with_rpv(rpv, fn):
    old = os.environ.get("DG_PQ_RPV")
    try:
        if rpv is None:
            os.environ.pop("DG_PQ_RPV", None)
        else:
            os.environ["DG_PQ_RPV"] = str(rpv)
        return fn()
    finally:
        if old is None:
            os.environ.pop("DG_PQ_RPV", None)
        else:
            os.environ["DG_PQ_RPV"] = old


def _same_bits(a, b):
    return (np.array_equal(a[1], b[1]) and
            np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)))


@pytest.mark.parametrize("metric", [dg.L2, dg.IP, dg.COSINE])
def test_list_length_edges(lens_index, metric):
    """nprobe=1: every list length in LENS is scanned by QPL queries."""
    case, idx, q_one, _ = lens_index(metric)
    gd, gi = idx.search(q_one, 10, nprobe=1)
    case.check(q_one, 10, 1, gd, gi)
    for r, l in enumerate(np.repeat(np.arange(len(LENS)), QPL)):
        assert (gi[r] >= 0).sum() == min(10, LENS[l])


@pytest.mark.parametrize("metric", [dg.L2, dg.IP])
@pytest.mark.parametrize("rpv", [6, 8, 16, 17])
def test_tile_variants_bit_identical(lens_index, metric, rpv):
    """The DG_PQ_RPV tiles add the same terms in the same order per (row,
    query): keys, and so results, must not differ from the default tile."""
    case, idx, q_one, q_all = lens_index(metric)
    for q, nprobe in ((q_one, 1), (q_all, len(LENS))):
        base = _with_rpv(None, lambda: idx.search(q, 10, nprobe=nprobe))
        var = _with_rpv(rpv, lambda: idx.search(q, 10, nprobe=nprobe))
        assert _same_bits(var, base)


@pytest.mark.parametrize("metric", [dg.L2, dg.IP])
def test_all_lists_33_queries(lens_index, metric):
    """nprobe == nlist: 33 queries on every list, nine rounds of the four
    waves, candidates of nine lists merged per query."""
    case, idx, _, q_all = lens_index(metric)
    gd, gi = idx.search(q_all, 10, nprobe=len(LENS))
    case.check(q_all, 10, len(LENS), gd, gi)


@pytest.mark.parametrize("metric", [dg.L2, dg.IP])
def test_three_nearest_lists(lens_index, metric):
    """nprobe=3 with queries between three centroids: the probe set is
    asserted clear in f64 (gap between the 3rd and 4th list)."""
    case, idx, _, _ = lens_index(metric)
    rng = np.random.default_rng(5)
    q = np.empty((12, case.d))
    for r in range(12):
        a, b, c = rng.permutation(len(LENS))[:3]
        q[r] = (0.5 * case.C[a] + 0.3 * case.C[b] + 0.2 * case.C[c] +
                rng.uniform(-0.5, 0.5, case.d))
    q = np.ascontiguousarray(q, np.float32)
    gd, gi = idx.search(q, 10, nprobe=3)
    case.check(q, 10, 3, gd, gi, min_gap=1.0)


@pytest.mark.parametrize("k", [1, 10, 100])
def test_k_values(lens_index, k):
    """k below, at and above the rows of the probed list (1, 3 and 255-row
    lists at k=100 leave -1 / 0.0 slots)."""
    case, idx, q_one, _ = lens_index(dg.L2)
    gd, gi = idx.search(q_one, k, nprobe=1)
    case.check(q_one, k, 1, gd, gi)


@pytest.mark.parametrize("nq", [1, 3])
def test_small_batch_replay(lens_index, nq):
    """nq <= 4 is the shape the graph replay path serves.  IVF-PQ stays out
    of it (its T build is a library GEMM): three calls of the ordinary path
    on reused workspaces, one answer, bit for bit."""
    case, idx, _, q_all = lens_index(dg.L2)
    q = q_all[5:5 + nq]
    out = [idx.search(q, 10, nprobe=len(LENS)) for _ in range(3)]
    assert _same_bits(out[1], out[0]) and _same_bits(out[2], out[0])
    case.check(q, 10, len(LENS), *out[0])


@pytest.mark.parametrize("metric", [dg.L2, dg.IP])
@pytest.mark.parametrize("d,m", [(16, 4), (48, 12), (32, 32)])
def test_subspace_counts(metric, d, m):
    """m=4: one code word per row; m=12: not a power of two (the % M of the
    S build, 3 words per row); m=32 at d=32: dsub=1."""
    lens = [300, 257, 40]
    case, lists, codes, x32 = _grouped_case(metric, d, m, lens, 77 + m)
    idx = case.new_index()
    try:
        _add_all(case, idx, lists, codes, x32)
        q = case.queries(np.repeat(np.arange(3), [4, 3, 2]))
        for nprobe in (1, 3):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


def test_insertion_order_and_ids():
    """Rows arrive shuffled across lists in two add calls with ids that are
    not positions: the code gather's permutation and the id lookup."""
    lens = [300, 257, 1025]
    case, lists, codes, x32 = _grouped_case(dg.L2, 32, 8, lens, 31)
    perm = case.rng.permutation(len(lists))
    lists, codes, x32 = lists[perm], codes[perm], x32[perm]
    ids = 7 * np.arange(len(lists), dtype=np.int64) + 3
    cut = 700
    idx = case.new_index()
    try:
        _add_all(case, idx, lists[:cut], codes[:cut], x32[:cut], ids[:cut])
        _add_all(case, idx, lists[cut:], codes[cut:],
                 np.ascontiguousarray(x32[cut:]), ids[cut:])
        q = case.queries(np.repeat(np.arange(3), 3))
        for nprobe in (1, 3):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


def test_filters_mask_and_mutation():
    """Filters, a list mask, tombstones and upserts on the PQ scan."""
    case, lists, codes, x32 = _grouped_case(dg.L2, 32, 8, LENS, 47)
    off = np.concatenate([[0], np.cumsum(LENS)])
    nl = len(LENS)
    idx = case.new_index()
    try:
        _add_all(case, idx, lists, codes, x32)
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


def test_centroids_replaced_after_codebooks():
    """S is built from centroids and codebooks: centroids set again under
    existing codebooks must rebuild it, not leave the first set's table."""
    lens = [300, 257, 40]
    case, lists, codes, x32 = _grouped_case(dg.L2, 32, 8, lens, 21)
    idx = dg.Index(dg.IVF_PQ, dg.L2, 32, nlist=3, m=8)
    try:
        idx.set_centroids(np.ascontiguousarray(case.cents32[::-1] * 0.5))
        idx.set_codebooks(case.cb32)
        idx.set_centroids(case.cents32)
        _add_all(case, idx, lists, codes, x32)
        q = case.queries(np.repeat(np.arange(3), 3))
        for nprobe in (1, 3):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


def test_list_mask_invalidates_small_batch_graph():
    """IVF-Flat replays a captured graph for nq <= 4; the graph holds the
    mask pointer of its capture, so setting or clearing a mask must force a
    recapture (found while adding the PQ mask case above)."""
    case = Case(dg.L2, 32, 8, 3, 11)
    lists = np.repeat(np.arange(3), [40, 50, 60])
    _, x32 = case.make_rows(lists)
    idx = dg.Index(dg.IVF_FLAT, dg.L2, 32, nlist=3)
    try:
        idx.set_centroids(case.cents32)
        idx.add(np.arange(len(lists), dtype=np.int64), x32)
        q = case.queries(np.array([0]))
        plain = [idx.search(q, 5, nprobe=3) for _ in range(3)]
        assert (plain[2][1] < 40).all()  # its own list is nearest
        idx.set_list_mask(np.array([0, 1, 1], np.uint8))
        masked = [idx.search(q, 5, nprobe=3) for _ in range(3)]
        for _, gi in masked:
            assert (gi >= 40).all(), gi
        idx.set_list_mask(None)
        assert _same_bits(idx.search(q, 5, nprobe=3), plain[0])
    finally:
        idx.close()


def test_m_limit():
    """m above the LDS limit is refused at create; the largest accepted m
    (dsub=4, nlist=2) passes A-D."""
    with pytest.raises(dg.DgError) as e:
        dg.Index(dg.IVF_PQ, dg.L2, 1024, nlist=16, m=256)
    assert e.value.status == 3  # DG_ENOT_SUPPORT
    m = dg.ivfpq_max_m()
    assert 96 <= m < 256 and m % 4 == 0
    assert str(m) in str(e.value)
    with pytest.raises(dg.DgError):
        dg.Index(dg.IVF_PQ, dg.L2, 4 * (m + 4), nlist=2, m=m + 4)
    case, lists, codes, x32 = _grouped_case(dg.L2, 4 * m, m, [257, 43], 9)
    idx = case.new_index()
    try:
        _add_all(case, idx, lists, codes, x32)
        q = case.queries(np.array([0, 0, 1, 1, 0]))
        for nprobe in (1, 2):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
        # a forced tile that cannot fit falls back to the default one
        big = _with_rpv(16, lambda: idx.search(q, 10, nprobe=2))
        assert _same_bits(big, (gd, gi))
    finally:
        idx.close()


def _scale_for_max_s(target):
    probe = Case(dg.L2, 32, 8, 3, 63)
    return float(np.sqrt(target / probe.S.max()))


def test_table_overflow_is_refused():
    """max S above the f16 range: set_codebooks fails loudly."""
    case = Case(dg.L2, 32, 8, 3, 63, scale=_scale_for_max_s(7.0e4))
    assert case.S.max() > HALF_MAX
    idx = dg.Index(dg.IVF_PQ, dg.L2, 32, nlist=3, m=8)
    try:
        idx.set_centroids(case.cents32)
        with pytest.raises(dg.DgError) as e:
            idx.set_codebooks(case.cb32)
        assert e.value.status == 3  # DG_ENOT_SUPPORT
        assert "65504" in str(e.value)
    finally:
        idx.close()


def test_tables_near_the_f16_limit():
    """max S about 6e4: the same checks hold, b scales with the data."""
    lens = [300, 257, 40]
    case, lists, codes, x32 = _grouped_case(
        dg.L2, 32, 8, lens, 63, scale=_scale_for_max_s(6.0e4))
    assert 5.9e4 < case.S.max() < HALF_MAX
    idx = case.new_index()
    try:
        _add_all(case, idx, lists, codes, x32)
        q = case.queries(np.repeat(np.arange(3), [4, 3, 2]))
        for nprobe in (1, 3):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()
