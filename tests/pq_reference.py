"""Float64 ADC reference for the IVF-PQ scan tests, ksub as a parameter.

The method is that of test_ivfpq_scan.py (read its header): rows are built
as centroid + known codewords + noise far below the codeword separation, the
construction is asserted unambiguous in f64, and the reference is
||q - (c_l + cb[codes])||^2 (q . (c_l + cb[codes]) for IP, the same on
normalized inputs for COSINE).

Tolerance, from the design and not from the kernel: each S and T entry is
rounded once to f16 (relative 2^-11), and the f32 work is R roundings,

  b_L2(q,row) = 2^-11 * sum_m(|S_m| + 2|T_m|)
                + R * 2^-24 * (sum_m(|S_m| + 2|T_m|) + ||q||^2 + 2|q.c|),
  b_IP(q,row) = 2^-11 * sum_m |T_m| + R * 2^-24 * (sum_m |T_m| + |q.c|),

with R = m + 3 at nbits = 8 (one add per subspace) and R = 2m + 3 at
nbits = 4 (up to two per subspace: the 4-bit scan may fold S - 2T into one
f32 table entry before it adds it).

Checks A-D and the 5 % strength condition are those of test_ivfpq_scan.py;
range_check compares a range search with the reference set.
"""
import numpy as np

import dingostore as dg

HALF_MAX = 65504.0
EPS16 = 2.0 ** -11
EPS32 = 2.0 ** -24
A_CENT = 6.0  # centroid norm in units of the codebook box side


def pack4(codes):
    """[n, m] codes < 16 -> [n, m/2] bytes, faiss's generic PQ packing:
    sub-quantizer 2j in the low nibble of byte j, 2j+1 in the high one."""
    codes = np.asarray(codes, np.uint8)
    assert codes.shape[1] % 2 == 0 and codes.max(initial=0) < 16
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def unpack4(packed, m):
    packed = np.asarray(packed, np.uint8).reshape(-1, m // 2)
    out = np.empty((len(packed), m), np.uint8)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


def _separated_box(rng, ksub, dim, sep):
    """ksub points of [-0.5, 0.5]^dim, pairwise at least sep apart."""
    pts = np.empty((ksub, dim))
    n = 0
    while n < ksub:
        c = rng.uniform(-0.5, 0.5, dim)
        if n == 0 or np.sqrt(((pts[:n] - c) ** 2).sum(1)).min() >= sep:
            pts[n] = c
            n += 1
    return pts


def _separated_sphere(rng, ksub, sep):
    """ksub unit vectors of R^3, pairwise at least sep apart."""
    pts = np.empty((ksub, 3))
    n = 0
    while n < ksub:
        c = rng.normal(size=3)
        c /= np.linalg.norm(c)
        if n == 0 or np.sqrt(((pts[:n] - c) ** 2).sum(1)).min() >= sep:
            pts[n] = c
            n += 1
    return pts


class Case:
    """Centroids, codebooks, rows with known (list, codes), and the f64
    model of the index: ids / lists / codes / alive of every row added."""

    def __init__(self, metric, d, m, nlist, seed, scale=1.0, nbits=4):
        self.metric, self.d, self.m, self.nlist = metric, d, m, nlist
        self.nbits = nbits
        self.ksub = ksub = 1 << nbits
        self.roundings = (2 * m + 3) if nbits == 4 else (m + 3)
        self.dsub = dsub = d // m
        self.scale = scale
        self.rng = rng = np.random.default_rng(seed)
        cents = np.zeros((nlist, d))
        cb = np.empty((m, ksub, dsub))
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
            bases = [_separated_sphere(rng, ksub, 0.1) * rho
                     for _ in range(4)]
            for j in range(m):
                cb[j, :, 0] = 0.0
                cb[j, :, 1:] = bases[j % 4][rng.permutation(ksub)]
        else:
            assert nlist <= d
            self.A = A_CENT * scale
            cents[np.arange(nlist), np.arange(nlist)] = self.A
            sep0 = 0.25 * float(ksub) ** (-1.0 / dsub)
            self.sep = sep0 * 0.8 * scale
            bases = [_separated_box(rng, ksub, dsub, sep0) for _ in range(4)]
            for j in range(m):  # permuted, mirrored, rescaled copies
                cb[j] = (bases[j % 4][rng.permutation(ksub)] *
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
        codes = rng.integers(0, self.ksub, (n, self.m)).astype(np.uint8)
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
        step = max(1, 4_000_000 // (m * self.ksub))
        cbn = (self.CB ** 2).sum(-1)  # [m, ksub]
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
                       m=self.m, nbits=self.nbits)
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
        acc = self.roundings * EPS32
        if self.metric == dg.L2:
            dist = ((q[None] - Y) ** 2).sum(1)
            sum_s = (Y ** 2).sum(1)  # sum_m S_m, all terms >= 0
            mag = sum_s + 2 * sum_t
            b = EPS16 * mag + acc * (mag + q @ q + 2 * qc)
            return dist, b, dist
        dist = Y @ q
        b = EPS16 * sum_t + acc * (sum_t + qc)
        return -dist, b, dist

    def eligible(self, q, nprobe, keep=None, mask=None, min_gap=None, r=0):
        """Rows one (normalized) query may return."""
        passes = self.alive.copy()
        if keep is not None:
            passes &= keep(self.ids)
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
        return passes & probed[self.lists]

    def assert_t_in_range(self, Q):
        # T stays inside f16 for these queries (f64 tables)
        tq = np.einsum("qmd,mkd->qmk", Q.reshape(len(Q), self.m, self.dsub),
                       self.CB)
        assert np.abs(tq).max() < HALF_MAX

    def check(self, q32, k, nprobe, gd, gi, keep=None, mask=None,
              min_gap=None):
        """Checks A-D for every query and the 5 % strength condition.
        keep: predicate on an id array (the filter); mask: list mask."""
        Q = self._unit(q32)
        self.assert_t_in_range(Q)
        assert gd.shape == gi.shape == (len(Q), k)
        kth, bmax = [], 0.0
        for r, q in enumerate(Q):
            elig = self.eligible(q, nprobe, keep, mask, min_gap, r)
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

    def exact_topk(self, q32, k, nprobe, keep=None, mask=None):
        """What a search without rounding returns (f64 reference order), in
        the index's output convention; lets check() be exercised, and the
        strength condition of a geometry asserted, without a device."""
        Q = self._unit(q32)
        gd = np.zeros((len(Q), k), np.float32)
        gi = np.full((len(Q), k), -1, np.int64)
        for r, q in enumerate(Q):
            cand = np.nonzero(self.eligible(q, nprobe, keep, mask, 0.0))[0]
            key, _, dist = self.reference(q)
            top = cand[np.argsort(key[cand], kind="stable")[:k]]
            gd[r, :len(top)] = dist[top]
            gi[r, :len(top)] = self.ids[top]
        return gd, gi

    def range_check(self, q32, radius, lims, gd, gi):
        """L2 range search over every list: the returned set is the
        reference set {dist < radius}, up to rows whose reference distance
        is within b of the radius; distances within b; ascending."""
        assert self.metric == dg.L2
        Q = self._unit(q32)
        self.assert_t_in_range(Q)
        assert len(lims) == len(Q) + 1 and lims[0] == 0
        assert lims[-1] == len(gd) == len(gi)
        sizes = []
        for r, q in enumerate(Q):
            cand = np.nonzero(self.alive)[0]
            _, b, dist = self.reference(q)
            by_id = dict(zip(self.ids[cand].tolist(), cand.tolist()))
            got = gi[lims[r]:lims[r + 1]].tolist()
            gdist = gd[lims[r]:lims[r + 1]].astype(np.float64)
            assert len(set(got)) == len(got) and all(g in by_id for g in got)
            rows = np.array([by_id[g] for g in got], np.int64)
            assert (np.abs(gdist - dist[rows]) <= b[rows]).all(), r
            assert (np.diff(gdist) >= 0).all(), r
            must = cand[dist[cand] < radius - b[cand]]
            may = cand[dist[cand] < radius + b[cand]]
            assert np.isin(must, rows).all(), r
            assert np.isin(rows, may).all(), r
            sizes.append(len(must))
        return sizes


def grouped_case(metric, d, m, lens, seed, scale=1.0, nbits=4):
    """Rows list by list, id == position."""
    case = Case(metric, d, m, len(lens), seed, scale, nbits)
    lists = np.repeat(np.arange(len(lens)), lens)
    codes, x32 = case.make_rows(lists)
    return case, lists, codes, x32


def add_all(case, idx, lists, codes, x32, ids=None):
    ids = np.arange(len(lists), dtype=np.int64) if ids is None else ids
    idx.add(ids, x32)
    case.record(ids, lists, codes)
